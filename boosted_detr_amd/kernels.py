"""Thin typed wrappers over the C ABI (include/bdetr.h).

PyTorch-ROCm tensors are used ONLY as device-memory containers (``data_ptr()``) and for the
current HIP stream; every arithmetic operation below is a hand-written HIP kernel in
``csrc/``.  There is no eager/PyTorch fallback: a missing library raises in ``_lib.lib()``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import BnAffine, BnBwdFuse, ConvDesc, GemmDesc, LossDesc, RowchainBwdDesc, RowchainFwdDesc, check

ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2


# Raw hipStream_t the kernels are launched on.  Asking torch for the current stream costs ~8 us per
# launch (a third of the host's enqueue time at ~1500 launches per step), so the training step pins
# the handle for its duration (engine.on_side_stream swaps it while side-stream work is queued).
_LAUNCH_STREAM = [None]


def set_launch_stream(handle: Optional[int]) -> Optional[int]:
    prev = _LAUNCH_STREAM[0]
    _LAUNCH_STREAM[0] = handle
    return prev


GEMM_FP32, GEMM_BF16X3, GEMM_MIXED, GEMM_SPLIT, GEMM_BF16X6 = 0, 1, 2, 3, 4
_GEMM_MODES = {"fp32": GEMM_FP32, "bf16x3": GEMM_BF16X3, "mixed": GEMM_MIXED, "split": GEMM_SPLIT, "bf16x6": GEMM_BF16X6}


def set_gemm_precision(mode) -> int:
    """Arithmetic of the conv/GEMM family: 'fp32' (exact fp32 MFMA everywhere), 'bf16x3' (split-bf16
    everywhere) or 'mixed' (default: exact forward, split-bf16 gradient products).  Returns the previous mode."""
    code = _GEMM_MODES.get(mode, mode)
    prev = _lib.lib().bdetr_get_gemm_precision()
    check(_lib.lib().bdetr_set_gemm_precision(int(code)), "set_gemm_precision")
    return prev


def get_gemm_precision() -> str:
    code = _lib.lib().bdetr_get_gemm_precision()
    return next(k for k, v in _GEMM_MODES.items() if v == code)


def demote_split_forward() -> None:
    """Frozen BatchNormalization (moving statistics) does not guarantee normalised activations, so the rest of this
    forward must not take the range-limited split-fp16 path: 'split' -> 'mixed' (exact-fp32 forward, same gradient
    arithmetic).  The enclosing ``gemm_precision`` scope restores the policy afterwards."""
    L = _lib.lib()
    if L.bdetr_get_gemm_precision() == GEMM_SPLIT:
        check(L.bdetr_set_gemm_precision(GEMM_MIXED), "set_gemm_precision")


# Deterministic mode (BDETR_DETERMINISTIC=1 or set_deterministic(True)): the only run-to-run variation of a training step is
# the ORDER in which float atomics land - the split-K slices of the weight gradients and the one-launch bias-gradient column
# sums.  In this mode the split-K launches store their slices into slabs of a workspace and a second launch folds them in a fixed
# order (the *_ws entry points of include/bdetr.h), and column sums take the two-level fixed-order reduction: two runs of the same
# step - eager or replayed from hipGraphs - give bit-identical weights.  Cost: one fold launch per split-K launch and the slabs'
# round trip through HBM (reported by bench.py as `deterministic_cost`).
import os as _os

_DETERMINISTIC = [_os.environ.get("BDETR_DETERMINISTIC", "0") == "1"]


def set_deterministic(on: bool) -> bool:
    prev = _DETERMINISTIC[0]
    _DETERMINISTIC[0] = bool(on)
    return prev


def deterministic() -> bool:
    return _DETERMINISTIC[0]


def _splitk_ws(rows: int, cols: int, sk: int, like: torch.Tensor):
    """(workspace tensor, its element count) of a deterministic split-K launch, or (None, 0).  Allocated from the caching allocator on
    the stream the launch goes to (side tasks run with the side stream current), so a later launch on that stream may reuse it."""
    if not _DETERMINISTIC[0] or sk <= 1:
        return None, 0
    n = int(_lib.lib().bdetr_splitk_workspace_elems(rows, cols, sk))
    return torch.empty(n, dtype=torch.float32, device=like.device), n


class gemm_precision:
    """``with gemm_precision('split'): ...`` - scoped arithmetic policy (None leaves it alone)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = set_gemm_precision(self.mode) if self.mode is not None else None
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            set_gemm_precision(self.prev)
        return False


def _stream() -> int:
    h = _LAUNCH_STREAM[0]
    return h if h is not None else torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _chk(*tensors, dtype=torch.float32):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.BdetrError("kernel operands must live in HBM (cuda tensors); no CPU path exists")
        if t.dtype != dtype:
            raise _lib.BdetrError(f"expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.BdetrError("kernel operands must be contiguous")


def empty(*shape, like: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    return torch.empty(shape, dtype=dtype, device=like.device)


# --------------------------------------------------------------------------------------
# K1
# --------------------------------------------------------------------------------------
def image_prep(image: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """backbone.py:49-56.  image [B,h,w,3] in [0,1] -> [B,H,W,4] (BGR - mean, pad channel 0)."""
    _chk(image)
    B, h, w, c = image.shape
    assert c == 3
    out = empty(B, H, W, 4, like=image)
    check(_lib.lib().bdetr_image_prep(_p(image), B, h, w, _p(out), H, W, _stream()), "image_prep")
    return out


def tokens_prepare(cat_ids: torch.Tensor, att_ids: torch.Tensor, C_: int, A: int):
    """tokenizers.py:40-82 for targets that are already int32 ids in HBM: (range-checked category ids [B,M],
    multi-hot attributes f32 [B,M,A])."""
    _chk(cat_ids, att_ids, dtype=torch.int32)
    if cat_ids.dim() == 3:
        cat_ids = cat_ids[..., 0].contiguous()
    B, M = cat_ids.shape
    slots = att_ids.shape[2] if att_ids.dim() == 3 else 1
    cat = torch.empty_like(cat_ids)
    hot = torch.empty((B, M, A), dtype=torch.float32, device=cat_ids.device)
    check(_lib.lib().bdetr_tokens_prepare(_p(cat_ids), _p(att_ids), B * M, slots, C_, A, _p(cat), _p(hot), _stream()), "tokens_prepare")
    return cat, hot


def augment(image: torch.Tensor, iparams: torch.Tensor, fparams: torch.Tensor, quality: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pipeline.py:274-341 on the GPU.  image [B,H,W,3]; iparams int32 [B,4]; fparams f32 [B,3]; quality int32 [B] or None
    (random_jpeg_quality between brightness and saturation, pipeline.py:319-325)."""
    _chk(image, fparams)
    _chk(iparams, dtype=torch.int32)
    B, H, W, c = image.shape
    assert c == 3
    L = _lib.lib()
    out = torch.empty_like(image)
    ws = empty(L.bdetr_augment_ws_floats(B), like=image)
    if quality is None:
        check(L.bdetr_augment(_p(image), _p(out), _p(iparams), _p(fparams), B, H, W, _p(ws), _stream()), "augment")
        return out
    _chk(quality, dtype=torch.int32)
    jws = torch.empty(int(L.bdetr_jpeg_quality_ws_bytes(B, H, W)), dtype=torch.uint8, device=image.device)
    check(L.bdetr_augment_jpeg(_p(image), _p(out), _p(iparams), _p(fparams), _p(quality), B, H, W, _p(ws), _p(jws), _stream()), "augment_jpeg")
    return out


def jpeg_quality(image: torch.Tensor, quality: torch.Tensor) -> torch.Tensor:
    """tf.image.adjust_jpeg_quality per image: float [B,H,W,3] in [0,1], quality int32 [B] (device)."""
    _chk(image)
    _chk(quality, dtype=torch.int32)
    B, H, W, c = image.shape
    assert c == 3 and quality.numel() == B
    L = _lib.lib()
    out = torch.empty_like(image)
    jws = torch.empty(int(L.bdetr_jpeg_quality_ws_bytes(B, H, W)), dtype=torch.uint8, device=image.device)
    check(L.bdetr_jpeg_quality(_p(image), _p(out), _p(quality), B, H, W, _p(jws), _stream()), "jpeg_quality")
    return out


# --------------------------------------------------------------------------------------
# convolution family
# --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConvGeom:
    N: int
    H: int
    W: int
    C: int
    K: int
    R: int
    S: int
    stride: int
    pad: int

    @property
    def OH(self) -> int:
        return (self.H + 2 * self.pad - self.R) // self.stride + 1

    @property
    def OW(self) -> int:
        return (self.W + 2 * self.pad - self.S) // self.stride + 1

    @property
    def M(self) -> int:
        return self.N * self.OH * self.OW

    def desc(self) -> ConvDesc:
        return ConvDesc(self.N, self.H, self.W, self.C, self.K, self.R, self.S, self.stride, self.pad, self.OH, self.OW)


# The fp32 path (csrc/igemm.hip, symbols bdetr_conv2d_*) and the pre-split path (csrc/sgemm.hip, bdetr_p16_conv2d_*) take the same
# arguments pass by pass; `family` is the symbol stem ("conv2d" / "p16_conv2d"), which the error texts carry too.
def _conv2d_fwd(family: str, x, w, bias, g: ConvGeom, act: int, want_stats: bool):
    _chk(x, w, bias)
    L = _lib.lib()
    d = g.desc()
    y = empty(g.N, g.OH, g.OW, g.K, like=x)
    psum = psq = None
    nparts = 0
    if want_stats:
        nparts = getattr(L, f"bdetr_{family}_fwd_stat_chunks")(C.byref(d))
        if nparts <= 0:
            check(-1, f"{family}_fwd_stat_chunks")
        psum = empty(nparts, g.K, like=x)
        psq = empty(nparts, g.K, like=x)
    check(getattr(L, f"bdetr_{family}_fwd")(_p(x), _p(w), _p(bias), _p(y), C.byref(d), act, _p(psum), _p(psq), _stream()), f"{family}_fwd")
    return y, (psum, psq, nparts)


def _conv2d_bwd_data(family: str, dy, w, g: ConvGeom, dx: Optional[torch.Tensor], accumulate: bool):
    _chk(dy, w, dx)
    d = g.desc()
    if dx is None:
        assert not accumulate
        dx = empty(g.N, g.H, g.W, g.C, like=dy)
    check(getattr(_lib.lib(), f"bdetr_{family}_bwd_data")(_p(dy), _p(w), _p(dx), C.byref(d), int(accumulate), _stream()), f"{family}_bwd_data")
    return dx


def _conv2d_bwd_weight(family: str, x, x_flags: tuple, dy, g: ConvGeom, dw: Optional[torch.Tensor], prezeroed: bool):
    """x_flags: what the family's entry point takes between x and dy (the pre-split one: whether x is the f16 pair)."""
    _chk(x, dy, dw)
    L = _lib.lib()
    d = g.desc()
    if dw is None:
        dw = empty(g.K, g.R, g.S, g.C, like=x)
        prezeroed = False
    sk = getattr(L, f"bdetr_{family}_bwd_weight_splitk")(C.byref(d))
    if sk > 1 and not prezeroed:
        check(L.bdetr_zero(_p(dw), dw.numel(), _stream()), "zero")
    ws, n = _splitk_ws(g.K, g.R * g.S * g.C, sk, x)
    check(getattr(L, f"bdetr_{family}_bwd_weight_ws")(_p(x), *x_flags, _p(dy), _p(dw), C.byref(d), sk, _p(ws), n, _stream()), f"{family}_bwd_weight")
    return dw


def conv2d_fwd(x, w, bias, g: ConvGeom, act: int = ACT_NONE, want_stats: bool = False):
    """x [N,H,W,C], w [K,R,S,C] (OHWI), bias [K] -> y [N,OH,OW,K] (+ partial column stats)."""
    return _conv2d_fwd("conv2d", x, w, bias, g, act, want_stats)


def conv2d_bwd_data(dy, w, g: ConvGeom, dx: Optional[torch.Tensor] = None, accumulate: bool = False):
    return _conv2d_bwd_data("conv2d", dy, w, g, dx, accumulate)


def conv2d_bwd_weight(x, dy, g: ConvGeom, dw: Optional[torch.Tensor] = None, prezeroed: bool = False):
    """prezeroed: dw already holds zeros (the optimizer's flat gradient buffer is cleared once per step),
    so the split-K atomics need no per-tensor memset."""
    return _conv2d_bwd_weight("conv2d", x, (), dy, g, dw, prezeroed)


# --------------------------------------------------------------------------------------
# pre-split (P16) operand path of the convolutions - csrc/sgemm.hip, csrc/p16.hip
# --------------------------------------------------------------------------------------
# A P16 tensor is carried as a float32 torch tensor of the logical shape (4 bytes per element, never read as
# floats): f16 pairs for forward operands, bf16 pairs for gradient operands (include/bdetr.h).
_OVERFLOW = [None]


def overflow_flag() -> torch.Tensor:
    """Device int32 the P16-f16 producers set when a value leaves the f16 pair's range (|x| >= 65504 / not finite)."""
    if _OVERFLOW[0] is None:
        _OVERFLOW[0] = torch.zeros(1, dtype=torch.int32, device="cuda")
    return _OVERFLOW[0]


_GUARD_ACTIVE = [True]


def set_guard_active(on: bool) -> None:
    """Whether the running step reads and clears the overflow flag (Model: policy 'split').  Only then do BatchNorm
    statistics watch it: under another policy nobody clears it, and a flag left up by an earlier guarded step (or by a stray
    p16_pack of a tool) would stop the moving-statistics updates for the rest of the process."""
    _GUARD_ACTIVE[0] = bool(on)


def flag_nonfinite(x: torch.Tensor) -> None:
    """Set the step's range guard when x holds a non-finite value (the loss vectors: a NaN born in a kernel without
    its own range check, e.g. the in-kernel split-fp16 products of the transformer layers)."""
    _chk(x)
    check(_lib.lib().bdetr_flag_nonfinite(_p(x), x.numel(), _p(overflow_flag()), _stream()), "flag_nonfinite")


def flag_snapshot(ordinal: torch.Tensor, host_ring: torch.Tensor) -> None:
    """Log the overflow flag against the step ordinal in a pinned int32[1 + n] host tensor: ordinal += 1 (device int32),
    host_ring[1 + ordinal % n] = flag, host_ring[0] = ordinal.  One lane on the launch stream, capturable, no D2H memcpy, no sync."""
    assert host_ring.dtype == torch.int32 and host_ring.numel() >= 2 and host_ring.is_pinned()
    assert ordinal.dtype == torch.int32 and ordinal.is_cuda
    check(_lib.lib().bdetr_flag_snapshot(_p(overflow_flag()), _p(ordinal), host_ring.data_ptr(), host_ring.numel() - 1, _stream()), "flag_snapshot")


def read_and_clear_overflow() -> bool:
    """Host read of the range guard (synchronises the device)."""
    f = overflow_flag()
    tripped = bool(int(f.item()))
    if tripped:
        f.zero_()
    return tripped


def p16_supported(g: ConvGeom) -> bool:
    d = g.desc()
    return bool(_lib.lib().bdetr_p16_supported(C.byref(d)))


def p16_pack(x, want_f16=True, want_bf16=True):
    """fp32 tensor (last dim % 8 == 0) -> (P16-f16 or None, P16-bf16 or None)."""
    _chk(x)
    f = torch.empty_like(x) if want_f16 else None
    b = torch.empty_like(x) if want_bf16 else None
    check(_lib.lib().bdetr_p16_pack(_p(x), x.numel(), _p(f), _p(b), _p(overflow_flag()) if want_f16 else None, _stream()), "p16_pack")
    return f, b


def p16_unpack(p, is_f16: bool):
    _chk(p)
    out = torch.empty_like(p)
    check(_lib.lib().bdetr_p16_unpack(_p(p), int(is_f16), p.numel(), _p(out), _stream()), "p16_unpack")
    return out


def p16_pack_conv_weights(w, want_fwd=True, want_bwd=True):
    """w [K,R,S,C] fp32 -> (P16-f16 [K,R,S,C] forward copy, P16-bf16 [C,R,S,K] transposed tap-flipped copy)."""
    _chk(w)
    K_, R, S, Cc = w.shape
    wf = torch.empty_like(w) if want_fwd else None
    wt = torch.empty((Cc, R, S, K_), dtype=torch.float32, device=w.device) if want_bwd else None
    check(_lib.lib().bdetr_p16_pack_conv_weights(_p(w), K_, R, S, Cc, _p(wf), _p(wt), _p(overflow_flag()) if want_fwd else None, _stream()),
          "p16_pack_conv_weights")
    return wf, wt


def bn_apply_p16(x2d, mean, rstd, gamma, beta, residual=None, relu=False, want_fp32=True, want_f16=True, want_bf16=True,
                 residual_p16=False, want_mask=False, residual_bn=None, even_pixels=None, zero_unwritten=False):
    """bn_apply with P16 outputs: returns (out32 | None, out_f16 | None, out_bf16 | None[, relu bit mask]).  residual_p16:
    `residual` is the f16 pair copy of the shortcut tensor.  residual_bn = (mean, rstd, gamma, beta): `residual` is the RAW
    output of the projection shortcut's convolution, normalised here.  want_mask: also return the 1-bit-per-element ReLU mask
    (int64 words) the backward pass of a residual unit reads instead of the forward output.
    even_pixels = (H, W): the rows are an [N, H, W] map of which only the pixels (2i, 2j) are read and written (the outputs keep
    their full shape; every other pixel and its mask words stay as allocated - or, with zero_unwritten, are zero-filled first: for
    diagnostics that fingerprint whole tensors).  The library refuses odd maps and C % 256 != 0."""
    _chk(x2d, mean, rstd, gamma, beta, residual)
    rbn = None
    if residual_bn is not None:
        _chk(*residual_bn)
        assert residual is not None and not residual_p16
        rbn = C.byref(BnAffine(*(_p(t) for t in residual_bn)))
        residual_p16 = 2
    rows, Cc = x2d.shape
    o32 = torch.empty_like(x2d) if want_fp32 else None
    of = torch.empty_like(x2d) if want_f16 else None
    ob = torch.empty_like(x2d) if want_bf16 else None
    mask = torch.empty(((rows * Cc // 4 + 63) // 64) * 4, dtype=torch.int64, device=x2d.device) if want_mask else None
    args = (_p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual), int(residual_p16), rbn, int(relu), _p(o32),
            _p(of), _p(ob), _p(mask), _p(overflow_flag()) if want_f16 else None, rows, Cc)
    if even_pixels is not None:
        H, W = even_pixels
        if zero_unwritten:
            for t in (o32, of, ob, mask.view(torch.float32) if mask is not None else None):
                if t is not None:
                    zero_(t)
        check(_lib.lib().bdetr_bn_apply_p16_even_pixels(*args, int(H), int(W), _stream()), "bn_apply_p16_even_pixels")
    else:
        check(_lib.lib().bdetr_bn_apply_p16(*args, _stream()), "bn_apply_p16")
    return (o32, of, ob, mask) if want_mask else (o32, of, ob)


def bn_bwd_p16(dout, out, x2d, mean, rstd, gamma, relu, frozen, want_residual_grad=False, dgamma=None, dbeta=None, beta=None, want_fp32=False,
               out_p16=False, pre=None, even_pixels=None, dout_compact=False):
    """bn_bwd writing the input gradient as a bf16 pair: returns (dx_bf16, dx32 | None, dgamma, dbeta, dres | None).
    out_p16: what the ReLU mask source `out` is - 0 / False the fp32 forward output, 1 / True its bf16 pair copy, 2 the bit
    mask of bn_apply_p16(want_mask=True)."""
    _chk(dout, x2d, mean, rstd, gamma, dgamma, dbeta)
    if out is not None and int(out_p16) != 2:
        _chk(out)
    L = _lib.lib()
    rows, Cc = x2d.shape
    dxb = torch.empty_like(x2d)
    dx32 = torch.empty_like(x2d) if want_fp32 else None
    dgamma = empty(Cc, like=x2d) if dgamma is None else dgamma
    dbeta = empty(Cc, like=x2d) if dbeta is None else dbeta
    dres = torch.empty_like(x2d) if want_residual_grad else None
    # pre = (part_g, part_gx, nparts): the reduction already done by the backward-data epilogue that produced dout
    ws = empty(2 * Cc * L.bdetr_bn_bwd_chunks(rows), like=x2d) if pre is None else None
    if even_pixels is not None and pre is None:
        # dout [N,H,W,C] is zero outside the pixels (2i, 2j) (ops.conv_bn tags such gradients): the reduction visits those only
        N, H, W = even_pixels
        assert N * H * W == rows
        # dout_compact: dout is the [N, H/2, W/2, C] tensor of the even pixels alone (the stride-2 backward-data products wrote it densely)
        assert not dout_compact or (dres is None and dout.numel() == N * (H // 2) * (W // 2) * Cc and H % 2 == 0 and W % 2 == 0)
        check(L.bdetr_bn_bwd_p16_even_pixels(_p(dout), _p(out), int(out_p16), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), int(relu), int(frozen),
                                             _p(dx32), _p(dxb), _p(dgamma), _p(dbeta), _p(dres), _p(ws), N, H, W, Cc, int(dout_compact), _stream()), "bn_bwd_p16_even_pixels")
        return dxb, dx32, dgamma, dbeta, dres
    assert not dout_compact, "a compact dout goes through the even-pixel reduction (even_pixels=(N, H, W), no pre)"
    pg, pgx, pn = pre if pre is not None else (None, None, 0)
    check(L.bdetr_bn_bwd_p16(_p(dout), _p(out), int(out_p16), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), int(relu), int(frozen), _p(dx32),
                             _p(dxb), _p(dgamma), _p(dbeta), _p(dres), _p(ws), _p(pg), _p(pgx), int(pn), rows, Cc, _stream()), "bn_bwd_p16")
    return dxb, dx32, dgamma, dbeta, dres


def p16_pack_conv_weights_multi(table: torch.Tensor) -> None:
    """table: int64 [n,7] device tensor of {w, w_f16, wt_bf16, K, R, S, C} rows."""
    _chk(table, dtype=torch.int64)
    check(_lib.lib().bdetr_p16_pack_conv_weights_multi(_p(table), table.shape[0], _p(overflow_flag()), _stream()), "p16_pack_conv_weights_multi")


def p16_conv2d_fwd(x_f16, w_f16, bias, g: ConvGeom, act: int = ACT_NONE, want_stats: bool = False):
    return _conv2d_fwd("p16_conv2d", x_f16, w_f16, bias, g, act, want_stats)


def p16_conv2d_bwd_data(dy_bf16, wt_bf16, g: ConvGeom, dx: Optional[torch.Tensor] = None, accumulate: bool = False):
    return _conv2d_bwd_data("p16_conv2d", dy_bf16, wt_bf16, g, dx, accumulate)


def relu_mask_apply_(x: torch.Tensor, relu_mask: torch.Tensor) -> torch.Tensor:
    """x <- x * relu_mask (bn_apply_p16's bit mask) in place."""
    _chk(x)
    _chk(relu_mask, dtype=torch.int64)
    check(_lib.lib().bdetr_relu_mask_apply(_p(x), _p(relu_mask), x.numel(), _stream()), "relu_mask_apply")
    return x


def p16_conv2d_bwd_data_masked_accum(dy_bf16, wt_bf16, g: ConvGeom, dx: torch.Tensor, relu_mask: torch.Tensor, bn_ctx=None, bn_ctx2=None, old_even=None):
    """dx (the gradient of a residual unit's output on entry) <- conv_transpose(dy) + dx * relu_mask, in place: the unit's skip
    branch merged inside the 1x1 backward-data epilogue of its first convolution.  bn_ctx = (y_prev, mean, rstd, gamma, beta,
    relu_mask_prev): the result is the complete output gradient of the PREVIOUS residual unit - also emit that unit's
    BatchNorm-backward partial sums; returns (dx, (part_g, part_gx, nparts)) then."""
    _chk(dy_bf16, wt_bf16, dx)
    _chk(relu_mask, dtype=torch.int64)
    L = _lib.lib()
    d = g.desc()
    if old_even is not None:
        # the unit's output gradient exists at the even pixels only: old_even [N, H/2, W/2, C] (compact), dx is a FRESH dense tensor
        _chk(old_even)
        assert bn_ctx2 is None and old_even.numel() * 4 == dx.numel() and g.H % 2 == 0 and g.W % 2 == 0

        def launch(fuse):
            check(L.bdetr_p16_conv2d_bwd_data_masked_accum_compact(_p(dy_bf16), _p(wt_bf16), _p(dx), _p(old_even), _p(relu_mask), C.byref(d), fuse, _stream()),
                  "p16_conv2d_bwd_data_masked_accum_compact")
    else:
        def launch(fuse):
            check(L.bdetr_p16_conv2d_bwd_data_masked_accum(_p(dy_bf16), _p(wt_bf16), _p(dx), _p(relu_mask), C.byref(d), fuse, _stream()),
                  "p16_conv2d_bwd_data_masked_accum")
    if bn_ctx is None:
        launch(None)
        return dx
    y_prev, mean, rstd, gamma, beta, bits_prev = bn_ctx
    _chk(y_prev, mean, rstd, gamma, beta)
    _chk(bits_prev, dtype=torch.int64)
    n = L.bdetr_p16_conv2d_bwd_data_stat_chunks(C.byref(d))
    if n <= 0:
        check(-1, "p16_conv2d_bwd_data_stat_chunks")
    pg, pgx = empty(n, g.C, like=dy_bf16), empty(n, g.C, like=dy_bf16)
    f = BnBwdFuse(_p(y_prev), _p(mean), _p(rstd), _p(gamma), _p(beta), 1, _p(pg), _p(pgx), _p(bits_prev))
    pgx2 = None
    if bn_ctx2 is not None:
        # the previous unit is a stage's FIRST one: its projection shortcut's BatchNorm sees the same gradient - (y0, mean0, rstd0):
        # also emit that BatchNorm's sum(g * xhat0); returns ((part_g, part_gx, n), (part_g, part_gx0, n))
        y0, mean0, rstd0 = bn_ctx2
        _chk(y0, mean0, rstd0)
        pgx2 = empty(n, g.C, like=dy_bf16)
        f.y2, f.mean2, f.rstd2, f.part_gx2 = _p(y0), _p(mean0), _p(rstd0), _p(pgx2)
    launch(C.byref(f))
    if pgx2 is not None:
        return dx, (pg, pgx, n), (pg, pgx2, n)
    return dx, (pg, pgx, n)


def p16_conv2d_bwd_data_bnstats(dy_bf16, wt_bf16, g: ConvGeom, y_prev, mean, rstd, gamma, beta, relu: bool):
    """Backward-data whose output is the gradient of the BatchNorm(+ReLU) output that fed this conv (pre-normalisation tensor
    y_prev, no residual): returns (dx, (part_g, part_gx, nparts)) - that layer's backward reduction, done in this epilogue."""
    _chk(dy_bf16, wt_bf16, y_prev, mean, rstd, gamma, beta)
    L = _lib.lib()
    d = g.desc()
    dx = empty(g.N, g.H, g.W, g.C, like=dy_bf16)
    n = L.bdetr_p16_conv2d_bwd_data_stat_chunks(C.byref(d))
    if n <= 0:
        check(-1, "p16_conv2d_bwd_data_stat_chunks")
    pg, pgx = empty(n, g.C, like=dy_bf16), empty(n, g.C, like=dy_bf16)
    f = BnBwdFuse(_p(y_prev), _p(mean), _p(rstd), _p(gamma), _p(beta), int(relu), _p(pg), _p(pgx), None)
    check(L.bdetr_p16_conv2d_bwd_data_bnstats(_p(dy_bf16), _p(wt_bf16), _p(dx), C.byref(d), C.byref(f), _stream()), "p16_conv2d_bwd_data_bnstats")
    return dx, (pg, pgx, n)


def p16_conv2d_bwd_weight(x_bf16, dy_bf16, g: ConvGeom, dw: Optional[torch.Tensor] = None, prezeroed: bool = False, x_f16: bool = False):
    """x_f16: `x_bf16` is the P16-f16 tensor the forward read (converted to bf16 pairs inside the kernel)."""
    return _conv2d_bwd_weight("p16_conv2d", x_bf16, (int(x_f16),), dy_bf16, g, dw, prezeroed)


# --------------------------------------------------------------------------------------
# GEMM
# --------------------------------------------------------------------------------------
def gemm_raw(I, J, R, a, lda, a_rc, b, ldb, b_rc, c, ldc, *, nb0=1, nb1=1, sa=(0, 0), sb=(0, 0), sc=(0, 0),
             bias=None, alpha=1.0, act=ACT_NONE, accumulate=False, splitk=1, grad=False):
    _chk(a, b, c, bias)
    g = GemmDesc(I, J, R, nb0, nb1, _p(a), lda, sa[0], sa[1], int(a_rc), _p(b), ldb, sb[0], sb[1], int(b_rc),
                 _p(c), ldc, sc[0], sc[1], _p(bias), float(alpha), act, int(accumulate), splitk, int(grad))
    ws, n = _splitk_ws(I, J, splitk, c) if ldc == J else (None, 0)
    check(_lib.lib().bdetr_gemm_ws(C.byref(g), _p(ws), n, _stream()), "gemm")
    return c


def gemm_grouped(descs):
    """descs: list of (I, J, R, a, lda, a_rc, b, ldb, b_rc, c, ldc, bias, act, accumulate); a product with an
    x-contiguous operand is a gradient product (dy @ w)."""
    arr = (GemmDesc * len(descs))()
    for k, (I, J, R, a, lda, a_rc, b, ldb, b_rc, c, ldc, bias, act, acc) in enumerate(descs):
        _chk(a, b, c, bias)
        arr[k] = GemmDesc(I, J, R, 1, 1, _p(a), lda, 0, 0, int(a_rc), _p(b), ldb, 0, 0, int(b_rc), _p(c), ldc, 0, 0, _p(bias), 1.0, act,
                          int(acc), 1, int(not (a_rc and b_rc)))
    check(_lib.lib().bdetr_gemm_grouped(arr, len(descs), _stream()), "gemm_grouped")


def linear_fwd_group(xs, ws, biases, act=ACT_NONE):
    """[x_k @ w_k^T + b_k for k]: same in/out widths, row counts may differ; one launch."""
    K_, O = xs[0].shape[1], ws[0].shape[0]
    ys = [empty(x.shape[0], O, like=x) for x in xs]
    gemm_grouped([(x.shape[0], O, K_, x, K_, True, w, K_, True, y, O, b, act, False) for x, w, b, y in zip(xs, ws, biases, ys)])
    return ys


def linear_bwd_data_group(dys, ws):
    """[dy_k @ w_k for k] in one launch."""
    O, K_ = ws[0].shape
    dxs = [empty(dy.shape[0], K_, like=dy) for dy in dys]
    gemm_grouped([(dy.shape[0], K_, O, dy, O, True, w, K_, False, dx, K_, None, ACT_NONE, False) for dy, w, dx in zip(dys, ws, dxs)])
    return dxs


def linear_fwd(x2d, w, bias, act=ACT_NONE):
    """y[m][o] = act(sum_i x[m][i] * w[o][i] + bias[o]);  w is [out][in]."""
    M, K = x2d.shape
    O = w.shape[0]
    y = empty(M, O, like=x2d)
    return gemm_raw(M, O, K, x2d, K, True, w, K, True, y, O, bias=bias, act=act)


def linear_bwd_data(dy2d, w, dx=None, accumulate=False):
    """dx[m][i] = sum_o dy[m][o] * w[o][i]."""
    M, O = dy2d.shape
    K = w.shape[1]
    if dx is None:
        dx = empty(M, K, like=dy2d)
    return gemm_raw(M, K, O, dy2d, O, True, w, K, False, dx, K, accumulate=accumulate, grad=True)


def _auto_splitk(I, J, R) -> int:
    cus = _lib.lib().bdetr_device_cus()
    tiles = max(1, ((I + 63) // 64) * ((J + 63) // 64))
    sk = max(1, min((2 * cus) // tiles, R // 128))      # floor: tiles x slices must not spill into a second round of workgroups
    return sk


def linear_bwd_weight(dy2d, x2d, dw=None, prezeroed: bool = False):
    """dw[o][i] = sum_m dy[m][o] * x[m][i]."""
    M, O = dy2d.shape
    K = x2d.shape[1]
    if dw is None:
        dw = empty(O, K, like=dy2d)
        prezeroed = False
    sk = _auto_splitk(O, K, M)
    if sk > 1 and not prezeroed:
        check(_lib.lib().bdetr_zero(_p(dw), dw.numel(), _stream()), "zero")
    return gemm_raw(O, K, M, dy2d, O, False, x2d, K, False, dw, K, splitk=sk, grad=True)


def linear_bwd_weight_group(dys, xs, dws, prezeroed):
    """dws[k][o][i] += sum_m dys[k][m][o] * xs[k][m][i] for up to 4 Dense layers of one shape in ONE split-K launch (float atomics);
    prezeroed[k]: dws[k] already holds zeros or a running sum.  Deterministic mode and ragged groups fall back to one launch each."""
    same = all(dy.shape == dys[0].shape and x.shape == xs[0].shape for dy, x in zip(dys, xs))
    if _DETERMINISTIC[0] or not same or len(dys) == 1 or len(dys) > 4:
        for dy, x, dw, pz in zip(dys, xs, dws, prezeroed):
            linear_bwd_weight(dy, x, dw=dw, prezeroed=pz)
        return dws
    M, O = dys[0].shape
    K_ = xs[0].shape[1]
    L = _lib.lib()
    for dw, pz in zip(dws, prezeroed):
        if not pz:
            check(L.bdetr_zero(_p(dw), dw.numel(), _stream()), "zero")
    tiles = len(dys) * max(1, ((O + 63) // 64) * ((K_ + 63) // 64))
    sk = max(1, min((2 * L.bdetr_device_cus()) // tiles, M // 128))
    arr = (GemmDesc * len(dys))()
    for k, (dy, x, dw) in enumerate(zip(dys, xs, dws)):
        _chk(dy, x, dw)
        arr[k] = GemmDesc(O, K_, M, 1, 1, _p(dy), O, 0, 0, 0, _p(x), K_, 0, 0, 0, _p(dw), K_, 0, 0, None, 1.0, ACT_NONE, 0, sk, 1)
    check(L.bdetr_gemm_grouped(arr, len(dys), _stream()), "gemm_grouped(weight gradients)")
    return dws


def colsum(x2d, out=None, prezeroed=False):
    """Column sums.  prezeroed: `out` already holds zeros (a slice of the step's zero-filled flat gradient buffer) - one
    launch that adds with float atomics instead of the two-kernel deterministic reduction."""
    _chk(x2d, out)
    L = _lib.lib()
    rows, cols = x2d.shape
    if prezeroed and out is not None and not _DETERMINISTIC[0]:
        check(L.bdetr_colsum_accumulate(_p(x2d), rows, cols, _p(out), _stream()), "colsum_accumulate")
        return out
    if out is None:
        out = empty(cols, like=x2d)
    ws = empty(L.bdetr_colsum_chunks(rows) * cols, like=x2d)
    check(L.bdetr_colsum(_p(x2d), rows, cols, _p(out), _p(ws), _stream()), "colsum")
    return out


def colsum_group(xs, outs):
    """out[m] += column sums of xs[m] for up to four [rows_m, cols] tensors of one width in ONE launch (float atomics: every out[m] must
    hold zeros or the running sum; the callers fall back to `colsum` per tensor in deterministic mode)."""
    _chk(*xs, *outs)
    n, cols = len(xs), xs[0].shape[1]
    assert 1 <= n <= 4 and all(x.dim() == 2 and x.shape[1] == cols for x in xs) and all(o.numel() == cols for o in outs)
    PA, LA = C.c_void_p * n, C.c_int64 * n
    check(_lib.lib().bdetr_colsum_accumulate_group(PA(*[x.data_ptr() for x in xs]), LA(*[x.shape[0] for x in xs]), cols, PA(*[o.data_ptr() for o in outs]), n,
                                                   _stream()), "colsum_accumulate_group")


# --------------------------------------------------------------------------------------
# BatchNorm
# --------------------------------------------------------------------------------------
def colstats(x2d):
    _chk(x2d)
    L = _lib.lib()
    rows, Cc = x2d.shape
    n = L.bdetr_bn_bwd_chunks(rows)
    psum, psq = empty(n, Cc, like=x2d), empty(n, Cc, like=x2d)
    check(L.bdetr_colstats(_p(x2d), rows, Cc, _p(psum), _p(psq), _stream()), "colstats")
    return psum, psq, n


def bn_stats(rows, Cc, parts, eps, momentum, bessel, moving_mean, moving_var, like):
    psum, psq, n = parts
    L = _lib.lib()
    mean, rstd = empty(Cc, like=like), empty(Cc, like=like)
    fold = L.bdetr_bn_stats_fold_rows()
    ws = empty(2 * fold * Cc, like=like) if n > 4 * fold else None
    check(L.bdetr_bn_stats(None, rows, Cc, _p(psum), _p(psq), n, eps, momentum, int(bessel), _p(mean), _p(rstd),
                           _p(moving_mean), _p(moving_var), _p(ws), _p(overflow_flag()) if _GUARD_ACTIVE[0] else None, _stream()), "bn_stats")
    return mean, rstd


def bn_stats_frozen(moving_mean, moving_var, eps):
    _chk(moving_mean, moving_var)
    Cc = moving_mean.numel()
    mean, rstd = empty(Cc, like=moving_mean), empty(Cc, like=moving_mean)
    check(_lib.lib().bdetr_bn_stats_frozen(_p(moving_mean), _p(moving_var), Cc, eps, _p(mean), _p(rstd), _stream()), "bn_stats_frozen")
    return mean, rstd


def bn_apply(x2d, mean, rstd, gamma, beta, residual=None, relu=False, out=None):
    _chk(x2d, mean, rstd, gamma, beta, residual, out)
    rows, Cc = x2d.shape
    if out is None:
        out = torch.empty_like(x2d)
    check(_lib.lib().bdetr_bn_apply(_p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual), int(relu), _p(out), rows, Cc, _stream()),
          "bn_apply")
    return out


def bn_bwd(dout, out, x2d, mean, rstd, gamma, relu, frozen, want_residual_grad=False, dgamma=None, dbeta=None, beta=None):
    _chk(dout, out, x2d, mean, rstd, gamma, dgamma, dbeta)
    L = _lib.lib()
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    dgamma = empty(Cc, like=x2d) if dgamma is None else dgamma
    dbeta = empty(Cc, like=x2d) if dbeta is None else dbeta
    dres = torch.empty_like(x2d) if want_residual_grad else None
    ws = empty(2 * Cc * L.bdetr_bn_bwd_chunks(rows), like=x2d)
    check(L.bdetr_bn_bwd(_p(dout), _p(out), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), int(relu), int(frozen), _p(dx), _p(dgamma), _p(dbeta),
                         _p(dres), _p(ws), rows, Cc, _stream()), "bn_bwd")
    return dx, dgamma, dbeta, dres


# ---- BatchNorm over row groups (csrc/groupnorm_rows.hip): x2d is [G * R, C], group g = rows [g R, (g + 1) R) ----
def bn_rows_stats(x2d, groups: int, eps):
    """Per-group batch statistics: (mean, rstd, var), each [G, C] (biased variance).  Raises the range guard for non-finite statistics."""
    _chk(x2d)
    rows, Cc = x2d.shape
    assert rows % groups == 0, (rows, groups)
    mean, rstd, var = empty(groups, Cc, like=x2d), empty(groups, Cc, like=x2d), empty(groups, Cc, like=x2d)
    check(_lib.lib().bdetr_bn_rows_stats(_p(x2d), groups, rows // groups, Cc, eps, _p(mean), _p(rstd), _p(var),
                                         _p(overflow_flag()) if _GUARD_ACTIVE[0] else None, _stream()), "bn_rows_stats")
    return mean, rstd, var


def bn_rows_apply(x2d, groups: int, mean, rstd, gamma, beta, var=None, momentum=0.0, moving_mean=None, moving_var=None):
    """out = gamma * (x - mean_g) * rstd_g + beta.  mean / rstd: [G, C] from bn_rows_stats, or [C] (moving statistics, shared by every
    group).  With moving_mean / moving_var (and var): the launch also folds the G groups' statistics into them in group order, as G
    sequential keras calls would - skipped while the range guard is up."""
    _chk(x2d, mean, rstd, gamma, beta, var, moving_mean, moving_var)
    rows, Cc = x2d.shape
    assert rows % groups == 0, (rows, groups)
    grouped = mean.dim() == 2
    out = torch.empty_like(x2d)
    check(_lib.lib().bdetr_bn_rows_apply(_p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(out), groups, rows // groups, Cc, int(grouped), _p(var),
                                         momentum, _p(moving_mean), _p(moving_var),
                                         _p(overflow_flag()) if (_GUARD_ACTIVE[0] and moving_mean is not None) else None, _stream()), "bn_rows_apply")
    return out


def bn_rows_bwd(dout, x2d, groups: int, mean, rstd, gamma, frozen, dgamma=None, dbeta=None):
    """(dx, dgamma, dbeta): dgamma / dbeta summed over all groups, dx from each row's own group (frozen: dx = g * rstd * gamma)."""
    _chk(dout, x2d, mean, rstd, gamma, dgamma, dbeta)
    rows, Cc = x2d.shape
    assert rows % groups == 0 and dout.shape == x2d.shape, (rows, groups)
    dx = torch.empty_like(x2d)
    dgamma = empty(Cc, like=x2d) if dgamma is None else dgamma
    dbeta = empty(Cc, like=x2d) if dbeta is None else dbeta
    ws = empty(2 * groups * Cc, like=x2d)
    check(_lib.lib().bdetr_bn_rows_bwd(_p(dout), _p(x2d), _p(mean), _p(rstd), _p(gamma), int(mean.dim() == 2), int(frozen), _p(dx), _p(dgamma), _p(dbeta),
                                       _p(ws), groups, rows // groups, Cc, _stream()), "bn_rows_bwd")
    return dx, dgamma, dbeta


# --------------------------------------------------------------------------------------
# pooling / softmax / layernorm / activations
# --------------------------------------------------------------------------------------
def maxpool_fwd(x):
    _chk(x)
    N, H, W, Cc = x.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = empty(N, OH, OW, Cc, like=x)
    check(_lib.lib().bdetr_maxpool3x3s2_fwd(_p(x), _p(y), N, H, W, Cc, OH, OW, _stream()), "maxpool_fwd")
    return y


def maxpool_bwd(x, y, dy):
    _chk(x, y, dy)
    N, H, W, Cc = x.shape
    _, OH, OW, _ = y.shape
    dx = torch.empty_like(x)
    check(_lib.lib().bdetr_maxpool3x3s2_bwd(_p(x), _p(y), _p(dy), _p(dx), N, H, W, Cc, OH, OW, _stream()), "maxpool_bwd")
    return dx


def stem_pool_fwd(y, mean, rstd, gamma, beta, want_fp32=False):
    """BatchNorm -> ReLU -> pad 1 -> MaxPool 3x3/2 of the raw stem convolution output y [N,H,W,C]: (pooled fp32 | None, pooled f16
    pair, tap bytes) - csrc/norm.hip stem_pool_fwd_kernel."""
    _chk(y, mean, rstd, gamma, beta)
    N, H, W, Cc = y.shape
    PH, PW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    o32 = empty(N, PH, PW, Cc, like=y) if want_fp32 else None
    of = empty(N, PH, PW, Cc, like=y)
    tap = torch.empty((N, PH, PW, Cc), dtype=torch.uint8, device=y.device)
    check(_lib.lib().bdetr_stem_pool_fwd(_p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), N, H, W, Cc, _p(o32), _p(of), _p(tap),
                                         _p(overflow_flag()), _stream()), "stem_pool_fwd")
    return o32, of, tap


def stem_pool_bwd(dpool, tap, y, mean, rstd, gamma, beta, dgamma=None, dbeta=None, dy_p16=False):
    """The backward of stem_pool_fwd + BatchNorm (batch statistics): (dy [N,H,W,C], dgamma, dbeta).  dy_p16: dy as the bf16 pair
    of the P16 layout (what stem_bwd_weight_s2d reads) instead of fp32 - same shape, never read as floats."""
    _chk(dpool, y, mean, rstd, gamma, beta, dgamma, dbeta)
    assert tap.is_cuda and tap.is_contiguous() and tap.dtype == torch.uint8 and tuple(tap.shape) == tuple(dpool.shape)
    L = _lib.lib()
    N, H, W, Cc = y.shape
    dy = torch.empty_like(y)
    dgamma = empty(Cc, like=y) if dgamma is None else dgamma
    dbeta = empty(Cc, like=y) if dbeta is None else dbeta
    ws = empty(2 * Cc * L.bdetr_stem_pool_bwd_chunks(N * H * W), like=y)
    check(L.bdetr_stem_pool_bwd(_p(dpool), _p(tap), _p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), N, H, W, Cc, _p(dy), int(dy_p16), _p(dgamma), _p(dbeta),
                                _p(ws), _stream()), "stem_pool_bwd")
    return dy, dgamma, dbeta


def stem_bwd_weight_s2d(x4, dy_bf16, dw):
    """dw [K,7,7,4] <- the weight gradient of the ResNet stem (7x7 / stride 2 / pad 3 over the 4-channel image x4 [N,H,W,4], H and W even)
    from dy's bf16 pair [N,H/2,W/2,K]: space-to-depth image pack, the pre-split XX kernel on a 4x4 / 16-channel view, unpack (include/bdetr.h)."""
    _chk(x4, dy_bf16, dw)
    L = _lib.lib()
    N, H, W, Cc = x4.shape
    Kout = dw.shape[0]
    assert Cc == 4 and H % 2 == 0 and W % 2 == 0 and tuple(dw.shape) == (Kout, 7, 7, 4) and tuple(dy_bf16.shape) == (N, H // 2, W // 2, Kout)
    x2 = empty(N, H // 2, W // 2, 16, like=x4)
    check(L.bdetr_p16_s2d_pack_bf16(_p(x4), N, H, W, _p(x2), _stream()), "p16_s2d_pack_bf16")
    dw2 = empty(Kout, 4, 4, 16, like=x4)
    check(L.bdetr_zero(_p(dw2), dw2.numel(), _stream()), "zero")
    check(L.bdetr_p16_stem_bwd_weight(_p(x2), _p(dy_bf16), _p(dw2), N, H // 2, W // 2, Kout, _stream()), "p16_stem_bwd_weight")
    check(L.bdetr_p16_s2d_unpack_dw(_p(dw2), _p(dw), Kout, _stream()), "p16_s2d_unpack_dw")
    return dw


ATTN_MASK_MULTIPLY, ATTN_MASK_EXCLUDE = 1, 2       # BDETR_ATTN_MASK_* of include/bdetr.h


def _attention_mask_args(mask, B, heads, nq, nk, like):
    """An attention mask [B or 1, h or 1, nq or 1, nk] -> (tensor whose pointer goes down, batch / head / query element strides with 0
    on a broadcast axis, rule).  float32: the multiply rule (K32); bool: exclusion (K33), handed down as uint8.  Anything else is
    a ValueError, raised before a launch."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError("attention mask must be a torch tensor")
    if mask.dim() != 4:
        raise ValueError(f"attention mask must be 4-D [B or 1, h or 1, q or 1, k], got shape {tuple(mask.shape)}")
    if mask.dtype not in (torch.float32, torch.bool):
        raise ValueError(f"attention mask must be float32 (multiply rule) or bool (exclusion rule), got {mask.dtype}")
    if mask.device != like.device:
        raise ValueError(f"attention mask lives on {mask.device}, the operands on {like.device}")
    mb, mh, mq, mk = mask.shape
    if mk != nk:
        raise ValueError(f"attention mask's last axis must be the full key length {nk}, got {mk}")
    for have, full, axis in ((mb, B, "batch"), (mh, heads, "head"), (mq, nq, "query")):
        if have != 1 and have != full:
            raise ValueError(f"attention mask's {axis} axis must be 1 or {full}, got {have}")
    if not mask.is_contiguous():
        raise ValueError("attention mask must be contiguous")
    sb = mh * mq * mk if mb != 1 else 0
    sh = mq * mk if mh != 1 else 0
    sq = mk if mq != 1 else 0
    if mask.dtype == torch.bool:
        return mask.view(torch.uint8), sb, sh, sq, ATTN_MASK_EXCLUDE
    return mask, sb, sh, sq, ATTN_MASK_MULTIPLY


def attention_fwd(q, k, v, heads, scale, mask=None):
    """q [B,nq,h*32], k/v [B,nk,h*32] -> o [B,h,nq,32], lse [B,h,nq] (fused; scores never hit HBM).

    mask (optional, a constant - no gradient is ever computed for it): [B or 1, h or 1, nq or 1, nk], contiguous.
      float32: the reference's rule, o = (softmax(scale q k^T) * mask) v with the softmax over all keys and lse that of the unmasked scores;
      bool:    exclusion - True attends, a False key takes no part in the softmax; lse runs over the kept keys; a row with no kept
               key gives o = 0 and lse = -inf.
    mask=None launches exactly the unmasked kernels."""
    _chk(q, k, v)
    B, nq, D = q.shape
    nk = k.shape[1]
    margs = None if mask is None else _attention_mask_args(mask, B, heads, nq, nk, q)
    o = empty(B, heads, nq, D // heads, like=q)
    lse = empty(B, heads, nq, like=q)
    if margs is None:
        check(_lib.lib().bdetr_attention_fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), B, heads, nq, nk, scale, _stream()), "attention_fwd")
    else:
        m, sb, sh, sq, rule = margs
        check(_lib.lib().bdetr_attention_masked_fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), B, heads, nq, nk, scale, _p(m), sb, sh, sq, rule,
                                                    _stream()), "attention_masked_fwd")
    return o, lse


def attention_bwd(q, k, v, o, d_o, lse, heads, scale, mask=None):
    """Gradients dq, dk, dv of attention_fwd; `mask` must be the forward's (it gets no gradient)."""
    _chk(q, k, v, o, d_o, lse)
    B, nq, D = q.shape
    nk = k.shape[1]
    margs = None if mask is None else _attention_mask_args(mask, B, heads, nq, nk, q)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = empty(B * heads * nq, like=q)
    if margs is None:
        check(_lib.lib().bdetr_attention_bwd(_p(q), _p(k), _p(v), _p(o), _p(d_o), _p(lse), _p(dq), _p(dk), _p(dv), _p(ws), B, heads, nq, nk,
                                             scale, _stream()), "attention_bwd")
    else:
        m, sb, sh, sq, rule = margs
        check(_lib.lib().bdetr_attention_masked_bwd(_p(q), _p(k), _p(v), _p(o), _p(d_o), _p(lse), _p(dq), _p(dk), _p(dv), _p(ws), B, heads, nq, nk,
                                                    scale, _p(m), sb, sh, sq, rule, _stream()), "attention_masked_bwd")
    return dq, dk, dv


def attention_mask_apply(x, mask, fill=False, out=None):
    """The mask of attention_fwd against a materialised contiguous [B,h,q,k] tensor (the unfused attention path, K34).
    fill=False: out = x * mask (float32 mask) or out = where(mask, x, 0) (bool mask);  fill=True (bool mask only): out = where(mask, x,
    a large finite negative), in front of softmax_rows_fwd.  out may be x."""
    _chk(x, out)
    B, heads, nq, nk = x.shape
    m, sb, sh, sq, rule = _attention_mask_args(mask, B, heads, nq, nk, x)
    if fill and rule != ATTN_MASK_EXCLUDE:
        raise ValueError("fill applies to a bool mask only")
    if out is None:
        out = torch.empty_like(x)
    check(_lib.lib().bdetr_attention_mask_apply(_p(x), _p(out), B, heads, nq, nk, _p(m), sb, sh, sq, rule, int(bool(fill)), _stream()),
          "attention_mask_apply")
    return out


def token_keep_host(region, h, w, r, c) -> np.ndarray:
    """The rule of token_key_mask (include/bdetr.h K35) on the host, NumPy int64: region [B,4] rows (top, left, height, width) in
    pixels of an h x w image -> bool [B, r*c], token (i, j) at i*c + j kept iff its centre lies in the region."""
    g = np.asarray(region).astype(np.int64).reshape(-1, 4)
    top, left, height, width = (g[:, k, None] for k in range(4))
    ci = (2 * np.arange(r, dtype=np.int64) + 1)[None, :] * np.int64(h)
    cj = (2 * np.arange(c, dtype=np.int64) + 1)[None, :] * np.int64(w)
    rows = (2 * r * top <= ci) & (ci < 2 * r * (top + height))
    cols = (2 * c * left <= cj) & (cj < 2 * c * (left + width))
    return (rows[:, :, None] & cols[:, None, :]).reshape(g.shape[0], r * c)


def token_key_mask(region, h, w, r, c):
    """region int32 [B,4] in HBM, rows (top, left, height, width) in pixels of an h x w image -> bool [B,1,1,r*c], the key mask of
    attention_fwd's exclusion rule over the tokens of an r x c feature grid: True where the token's centre lies in the region
    (include/bdetr.h K35).  One launch that reads `region` on the device; nothing is read back."""
    _chk(region, dtype=torch.int32)
    if region.dim() != 2 or region.shape[1] != 4:
        raise ValueError(f"region must be int32 [B,4], got shape {tuple(region.shape)}")
    B = region.shape[0]
    mask = torch.empty((B, int(r) * int(c)), dtype=torch.uint8, device=region.device)
    check(_lib.lib().bdetr_token_key_mask(_p(region), B, int(h), int(w), int(r), int(c), _p(mask), _stream()), "token_key_mask")
    return mask.view(torch.bool).view(B, 1, 1, int(r) * int(c))


def softmax_rows_fwd(s2d, scale=1.0, out=None):
    _chk(s2d, out)
    rows, cols = s2d.shape
    if out is None:
        out = torch.empty_like(s2d)
    check(_lib.lib().bdetr_softmax_rows_fwd(_p(s2d), _p(out), rows, cols, scale, _stream()), "softmax_fwd")
    return out


def softmax_rows_bwd(p2d, dp2d, scale=1.0, out=None):
    _chk(p2d, dp2d, out)
    rows, cols = p2d.shape
    if out is None:
        out = torch.empty_like(p2d)
    check(_lib.lib().bdetr_softmax_rows_bwd(_p(p2d), _p(dp2d), _p(out), rows, cols, scale, _stream()), "softmax_bwd")
    return out


def add_dropout_layernorm_fwd(x2d, y2d, gamma, beta, eps, rate=0.0, seed=0, seed_base=None):
    """seed_base: device int64 [1] holding the per-step seed (folded into `seed` on the device)."""
    _chk(x2d, y2d, gamma, beta)
    rows, D = x2d.shape
    out = torch.empty_like(x2d)
    mean, rstd = empty(rows, like=x2d), empty(rows, like=x2d)
    check(_lib.lib().bdetr_add_dropout_layernorm_fwd(_p(x2d), _p(y2d), _p(gamma), _p(beta), _p(out), _p(mean), _p(rstd), rows, D, eps, rate,
                                                     seed, _p(seed_base), _stream()), "add_dropout_layernorm_fwd")
    return out, mean, rstd


def add_dropout_layernorm_bwd(dout, x2d, y2d, gamma, mean, rstd, rate=0.0, seed=0, dgamma=None, dbeta=None, seed_base=None):
    _chk(dout, x2d, y2d, gamma, mean, rstd, dgamma, dbeta)
    L = _lib.lib()
    rows, D = x2d.shape
    dx, dy = torch.empty_like(x2d), torch.empty_like(x2d)
    dgamma = empty(D, like=x2d) if dgamma is None else dgamma
    dbeta = empty(D, like=x2d) if dbeta is None else dbeta
    ws = empty(2 * D * L.bdetr_ln_bwd_chunks(rows), like=x2d)
    check(L.bdetr_add_dropout_layernorm_bwd(_p(dout), _p(x2d), _p(y2d), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dy), _p(dgamma), _p(dbeta),
                                            _p(ws), rows, D, rate, seed, _p(seed_base), 0, _stream()), "add_dropout_layernorm_bwd")
    return dx, dy, dgamma, dbeta


# --------------------------------------------------------------------------------------
# row chain (csrc/rowchain.hip): out-projection + LayerNorm (+ FFN + LayerNorm) of a transformer layer in one launch
# --------------------------------------------------------------------------------------
ROWCHAIN_WIDTH = 256


def rowchain_pack_weights(table: torch.Tensor) -> None:
    """table: int64 [n,3] device tensor of {W [256,256] fp32, forward copy | 0, backward copy | 0} rows."""
    _chk(table, dtype=torch.int64)
    check(_lib.lib().bdetr_rowchain_pack_weights(_p(table), table.shape[0], _p(overflow_flag()), _stream()), "rowchain_pack_weights")


def rowchain_fwd(ctx2d, resid2d, packs, biases, ln1, ln2, eps, rate, seed1, seed2, seed_base):
    """packs / biases: 1 or 3 packed forward copies / bias vectors (Wo[, W1, W2]); ln1 / ln2: (gamma, beta) value tensors (ln2 None for
    one stage).  Returns a dict of the outputs and saved tensors."""
    n = len(packs)
    _chk(ctx2d, resid2d, *biases, *ln1, *(ln2 or ()))
    M, D = ctx2d.shape
    assert D == ROWCHAIN_WIDTH and n in (1, 3) and resid2d.shape == ctx2d.shape
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=ctx2d.device)
    o = {"pre1": e(M, D), "x1": e(M, D), "mean1": e(M), "rstd1": e(M)}
    if n == 3:
        o.update({"h": e(M, D), "pre2": e(M, D), "x2": e(M, D), "mean2": e(M), "rstd2": e(M)})
    d = RowchainFwdDesc()
    d.M, d.nstages, d.eps, d.rate = M, n, float(eps), float(rate)
    d.ctx, d.resid = _p(ctx2d), _p(resid2d)
    for k in range(n):
        d.w[k], d.bias[k] = _p(packs[k]), _p(biases[k])
    d.g1, d.b1 = _p(ln1[0]), _p(ln1[1])
    if n == 3:
        d.g2, d.b2 = _p(ln2[0]), _p(ln2[1])
    for k, v in o.items():
        setattr(d, k, _p(v))
    d.seed1, d.seed2, d.seed_base = int(seed1), int(seed2), _p(seed_base)
    check(_lib.lib().bdetr_rowchain_fwd(C.byref(d), _stream()), "rowchain_fwd")
    return o


def rowchain_bwd(dout2d, saved, packs_t, gammas, rate, seed1, seed2, seed_base):
    """saved: rowchain_fwd's dict; packs_t: the packed backward copies; gammas: (gamma1[, gamma2]).  Returns (dctx, dresid, [G0, G1, G2],
    partials, nparts)."""
    n = len(packs_t)
    _chk(dout2d)
    M, D = dout2d.shape
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dout2d.device)
    L = _lib.lib()
    nparts = L.bdetr_rowchain_partial_rows(M)
    G = [e(M, D) for _ in range(n)]
    dctx, dresid, partials = e(M, D), e(M, D), e(nparts, 7, D)
    d = RowchainBwdDesc()
    d.M, d.nstages, d.rate, d.dout = M, n, float(rate), _p(dout2d)
    d.pre1, d.mean1, d.rstd1, d.g1 = _p(saved["pre1"]), _p(saved["mean1"]), _p(saved["rstd1"]), _p(gammas[0])
    if n == 3:
        d.pre2, d.mean2, d.rstd2, d.g2, d.h = _p(saved["pre2"]), _p(saved["mean2"]), _p(saved["rstd2"]), _p(gammas[1]), _p(saved["h"])
        d.G1, d.G2 = _p(G[1]), _p(G[2])
    for k in range(n):
        d.wt[k] = _p(packs_t[k])
    d.G0, d.dresid, d.dctx, d.partials = _p(G[0]), _p(dresid), _p(dctx), _p(partials)
    d.seed1, d.seed2, d.seed_base = int(seed1), int(seed2), _p(seed_base)
    check(L.bdetr_rowchain_bwd(C.byref(d), _stream()), "rowchain_bwd")
    return dctx, dresid, G, partials, nparts


def rowchain_reduce(partials, nparts, dsts, accumulate):
    """dsts: 7 tensors or None ({dgamma2, dbeta2, dbias2, dbias1, dgamma1, dbeta1, dbias0}); accumulate: 7 flags."""
    ptrs = (C.c_void_p * 7)(*[_p(t) for t in dsts])
    acc = (C.c_int * 7)(*[int(bool(a)) for a in accumulate])
    check(_lib.lib().bdetr_rowchain_reduce(_p(partials), nparts, C.byref(ptrs), C.byref(acc), _stream()), "rowchain_reduce")


def _unary(name, x, out=None):
    _chk(x, out)
    if out is None:
        out = torch.empty_like(x)
    check(getattr(_lib.lib(), name)(_p(x), _p(out), x.numel(), _stream()), name)
    return out


def _binary(name, a, b, out=None):
    _chk(a, b, out)
    if out is None:
        out = torch.empty_like(a)
    check(getattr(_lib.lib(), name)(_p(a), _p(b), _p(out), a.numel(), _stream()), name)
    return out


def sigmoid_fwd(x): return _unary("bdetr_sigmoid_fwd", x)
def sigmoid_bwd(y, dy): return _binary("bdetr_sigmoid_bwd", y, dy)
def boxsigmoid_fwd(x): return _unary("bdetr_boxsigmoid_fwd", x)
def boxsigmoid_bwd(y, dy): return _binary("bdetr_boxsigmoid_bwd", y, dy)
def tanh_bwd(y, dy): return _binary("bdetr_tanh_bwd", y, dy)
def relu_bwd(y, dy): return _binary("bdetr_relu_bwd", y, dy)
def add(a, b, out=None): return _binary("bdetr_add", a, b, out)


def zero_(t):
    _chk(t)
    check(_lib.lib().bdetr_zero(_p(t), t.numel(), _stream()), "zero")
    return t


def axpy_(alpha, x, y):
    _chk(x, y)
    check(_lib.lib().bdetr_axpy(float(alpha), _p(x), _p(y), x.numel(), _stream()), "axpy")
    return y


def add_bcast_rows(a, row):
    """a [B, *rest] + row [*rest]"""
    _chk(a, row)
    out = torch.empty_like(a)
    rowlen = row.numel()
    check(_lib.lib().bdetr_add_bcast_rows(_p(a), _p(row), _p(out), a.numel() // rowlen, rowlen, _stream()), "add_bcast_rows")
    return out


def sum_over_batch(x, n, out=None):
    _chk(x, out)
    if out is None:
        out = empty(n, like=x)
    check(_lib.lib().bdetr_sum_over_batch(_p(x), _p(out), x.numel() // n, n, 0, _stream()), "sum_over_batch")
    return out


# --------------------------------------------------------------------------------------
# set criterion
# --------------------------------------------------------------------------------------
def loss_desc(B, M, N, Cc, A, category_weight, attribute_weight, box_weight, exist_weight) -> LossDesc:
    return LossDesc(B, M, N, Cc, A, category_weight, attribute_weight, box_weight, exist_weight)


def cost_matrix(d: LossDesc, cat_pred, att_pred, box_pred, cat_ids, att_hot, bbox, num_objects, components=False, period=None):
    """period: the predictions are d.B = L * period images (several calls stacked), the targets `period` images (bdetr_cost_matrix_tiled)."""
    _chk(cat_pred, att_pred, box_pred, att_hot, bbox)
    _chk(cat_ids, num_objects, dtype=torch.int32)
    if period is not None:
        assert not components and d.B % period == 0 and cat_ids.shape[0] == period and num_objects.numel() == period
        cost = empty(d.B, d.M, d.N, like=cat_pred)
        check(_lib.lib().bdetr_cost_matrix_tiled(C.byref(d), period, _p(cat_pred), _p(att_pred), _p(box_pred), _p(cat_ids), _p(att_hot), _p(bbox),
                                                 _p(num_objects), _p(cost), _stream()), "cost_matrix_tiled")
        return cost
    cost = empty(d.B, d.M, d.N, like=cat_pred)
    comps = [empty(d.B, d.M, d.N, like=cat_pred) for _ in range(3)] if components else [None] * 3
    check(_lib.lib().bdetr_cost_matrix(C.byref(d), _p(cat_pred), _p(att_pred), _p(box_pred), _p(cat_ids), _p(att_hot), _p(bbox),
                                       _p(num_objects), _p(cost), _p(comps[0]), _p(comps[1]), _p(comps[2]), _stream()), "cost_matrix")
    return (cost, comps) if components else cost


def lsa(cost, num_objects, period=None):
    _chk(cost)
    _chk(num_objects, dtype=torch.int32)
    B, M, N = cost.shape
    match = empty(B, M, like=cost, dtype=torch.int32)
    if period is not None:
        assert B % period == 0 and num_objects.numel() == period
        check(_lib.lib().bdetr_lsa_tiled(_p(cost), _p(num_objects), B, period, M, N, _p(match), _stream()), "lsa_tiled")
        return match
    check(_lib.lib().bdetr_lsa(_p(cost), _p(num_objects), B, M, N, _p(match), _stream()), "lsa")
    return match


def match_to_mask(match, N):
    _chk(match, dtype=torch.int32)
    B, M = match.shape
    mask = empty(B, M, N, like=match, dtype=torch.float32)
    check(_lib.lib().bdetr_match_to_mask(_p(match), _p(mask), B, M, N, _stream()), "match_to_mask")
    return mask


def set_loss(d: LossDesc, cat_pred, att_pred, box_pred, cat_ids, att_hot, bbox, num_objects, match, loss_scale=1.0, want_grads=True, period=None):
    _chk(cat_pred, att_pred, box_pred, att_hot, bbox)
    _chk(cat_ids, num_objects, match, dtype=torch.int32)
    losses = empty(6, d.B, like=cat_pred)
    d_cat = torch.empty_like(cat_pred) if want_grads else None
    d_att = torch.empty_like(att_pred) if (want_grads and att_pred is not None) else None
    d_box = torch.empty_like(box_pred) if want_grads else None
    if period is not None:
        assert d.B % period == 0 and cat_ids.shape[0] == period and num_objects.numel() == period
        check(_lib.lib().bdetr_set_loss_tiled(C.byref(d), period, _p(cat_pred), _p(att_pred), _p(box_pred), _p(cat_ids), _p(att_hot), _p(bbox),
                                              _p(num_objects), _p(match), _p(losses), _p(d_cat), _p(d_att), _p(d_box), float(loss_scale), _stream()),
              "set_loss_tiled")
        return losses, d_cat, d_att, d_box
    check(_lib.lib().bdetr_set_loss(C.byref(d), _p(cat_pred), _p(att_pred), _p(box_pred), _p(cat_ids), _p(att_hot), _p(bbox), _p(num_objects),
                                    _p(match), _p(losses), _p(d_cat), _p(d_att), _p(d_box), float(loss_scale), _stream()), "set_loss")
    return losses, d_cat, d_att, d_box


# --------------------------------------------------------------------------------------
# detection metric - csrc/detmetric.hip
# --------------------------------------------------------------------------------------
def det_postprocess(cat_pred):
    """cat_pred [B,N,C] probabilities -> (score f32 [B,N], label int32 [B,N]): first-max argmax over classes 2 .. C-1."""
    _chk(cat_pred)
    B, N, Cc = cat_pred.shape
    score = empty(B, N, like=cat_pred)
    label = empty(B, N, like=cat_pred, dtype=torch.int32)
    check(_lib.lib().bdetr_det_postprocess(_p(cat_pred), B, N, Cc, _p(score), _p(label), _stream()), "det_postprocess")
    return score, label


def _match_outputs(score, thresholds, A=None):
    """What the five match wrappers share: the host thresholds as contiguous fp64, and the outputs, allocated like score [B,N].
    Returns (thr, T, order, class_rank, tp_bits, ig_bits, matched_gt); the per-range outputs gain a leading A when A is given
    (the COCO kernels), otherwise class_rank and ig_bits are None."""
    B, N = score.shape
    thr = np.ascontiguousarray(thresholds, np.float64).reshape(-1)
    T = int(thr.size)
    lead = () if A is None else (max(A, 1),)
    order = empty(B, N, like=score, dtype=torch.int32)
    class_rank = None if A is None else empty(B, N, like=score, dtype=torch.int32)
    tp_bits = empty(*lead, B, N, like=score, dtype=torch.int16)
    ig_bits = None if A is None else empty(*lead, B, N, like=score, dtype=torch.int16)
    matched = empty(*lead, B, max(T, 1), N, like=score, dtype=torch.int32)
    return thr, T, order, class_rank, tp_bits, ig_bits, matched


def det_match(score, label, box_pred, gt_label, gt_box, num_objects, thresholds, num_classes: int, max_dets: int, gt_count):
    """COCOeval's matching of one batch (include/bdetr.h, K14).  thresholds: host fp64 values; gt_count: int32 [num_classes] in HBM,
    the batch's per-class ground-truth counts are added to it.  Returns (order int32 [B,N], tp_bits int16 [B,N] - the uint16 bit
    pattern, torch has no arithmetic on uint16 - and matched_gt int32 [B,T,N])."""
    _chk(score, box_pred, gt_box)
    _chk(label, gt_label, num_objects, gt_count, dtype=torch.int32)
    B, N = score.shape
    M = gt_label.shape[1]
    if tuple(label.shape) != (B, N) or tuple(box_pred.shape) != (B, N, 4) or tuple(gt_label.shape) != (B, M) or tuple(gt_box.shape) != (B, M, 4) \
            or num_objects.numel() != B or gt_count.numel() != num_classes:
        raise _lib.BdetrError("det_match: operand shapes disagree")
    thr, T, order, _, tp_bits, _, matched = _match_outputs(score, thresholds)
    check(_lib.lib().bdetr_det_match(_p(score), _p(label), _p(box_pred), _p(gt_label), _p(gt_box), _p(num_objects), thr.ctypes.data, B, N, M,
                                     int(num_classes), T, int(max_dets), _p(order), _p(tp_bits), _p(matched), _p(gt_count), _stream()), "det_match")
    return order, tp_bits, matched


# --------------------------------------------------------------------------------------
# mask metric - csrc/maskmetric.hip
# --------------------------------------------------------------------------------------
def _dtypes(what: str, **named):
    """Each operand against its dtype, by name, before anything else is looked at (the message says which one)."""
    for name, (t, dtype) in named.items():
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise _lib.BdetrError(f"{what}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t).__name__)}")


def mask_binarize(x, threshold: float):
    """x [..., P] fp32 -> (bits int64 [..., ceil(P/64)], area int32 [...]): bit p mod 64 of word p div 64 is x[p] > threshold (NaN:
    false), the tail word's unused bits are zero, area = the row's set bits.  int64 holds the uint64 bit pattern (torch has no
    arithmetic on uint64).  Mask logits are cut at 0.0 (sigmoid > 0.5), [0,1] targets at 0.5."""
    _dtypes("mask_binarize", x=(x, torch.float32))
    if x.dim() < 1 or x.numel() == 0:
        raise _lib.BdetrError(f"mask_binarize: x must be [..., P] with at least one element, got {tuple(x.shape)}")
    _chk(x)
    P = x.shape[-1]
    lead = tuple(x.shape[:-1])
    bits = empty(*lead, (P + 63) // 64, like=x, dtype=torch.int64)
    area = empty(*lead, like=x, dtype=torch.int32)
    check(_lib.lib().bdetr_mask_binarize(_p(x), x.numel() // P, P, float(threshold), _p(bits), _p(area), _stream()), "mask_binarize")
    return bits, area


def mask_match(score, label, det_bits, det_area, gt_label, gt_bits, gt_area, num_objects, thresholds, num_classes: int, max_dets: int, gt_count):
    """det_match with packed masks in place of the boxes (include/bdetr.h, K15): det_bits int64 [B,N,W] / det_area int32 [B,N] and
    gt_bits int64 [B,M,W] / gt_area int32 [B,M] as mask_binarize returns them.  Everything else, and the returned
    (order, tp_bits, matched_gt), as det_match."""
    _dtypes("mask_match", score=(score, torch.float32), label=(label, torch.int32), det_bits=(det_bits, torch.int64),
            det_area=(det_area, torch.int32), gt_label=(gt_label, torch.int32), gt_bits=(gt_bits, torch.int64), gt_area=(gt_area, torch.int32),
            num_objects=(num_objects, torch.int32), gt_count=(gt_count, torch.int32))
    if score.dim() != 2 or gt_label.dim() != 2 or det_bits.dim() != 3:
        raise _lib.BdetrError("mask_match: operand shapes disagree (score [B,N], gt_label [B,M], det_bits [B,N,W])")
    B, N = score.shape
    M, W = gt_label.shape[1], det_bits.shape[2]
    if tuple(label.shape) != (B, N) or tuple(det_bits.shape) != (B, N, W) or tuple(det_area.shape) != (B, N) or tuple(gt_label.shape) != (B, M) \
            or tuple(gt_bits.shape) != (B, M, W) or tuple(gt_area.shape) != (B, M) or num_objects.numel() != B or gt_count.numel() != num_classes:
        raise _lib.BdetrError("mask_match: operand shapes disagree")
    _chk(score)
    _chk(label, det_area, gt_label, gt_area, num_objects, gt_count, dtype=torch.int32)
    _chk(det_bits, gt_bits, dtype=torch.int64)
    thr, T, order, _, tp_bits, _, matched = _match_outputs(score, thresholds)
    check(_lib.lib().bdetr_mask_match(_p(score), _p(label), _p(det_bits), _p(det_area), _p(gt_label), _p(gt_bits), _p(gt_area), _p(num_objects),
                                      thr.ctypes.data, B, N, M, W, int(num_classes), T, int(max_dets), _p(order), _p(tp_bits), _p(matched),
                                      _p(gt_count), _stream()), "mask_match")
    return order, tp_bits, matched


# --------------------------------------------------------------------------------------
# the full COCO protocol - csrc/detmetric.hip (K16), csrc/maskmetric.hip (K17)
# --------------------------------------------------------------------------------------
def _coco_operands(what: str, B: int, M: int, gt_crowd, gt_area, image_hw, area_ranges, gt_count, num_classes: int) -> int:
    """The operands K16 and K17 share, checked; returns A."""
    _dtypes(what, gt_crowd=(gt_crowd, torch.uint8), image_hw=(image_hw, torch.int32), area_ranges=(area_ranges, torch.float64),
            gt_count=(gt_count, torch.int32))
    if gt_area is not None:
        _dtypes(what, gt_area=(gt_area, torch.float32))
        if tuple(gt_area.shape) != (B, M):
            raise _lib.BdetrError(f"{what}: gt_area must be [B,M]")
        _chk(gt_area)
    if tuple(gt_crowd.shape) != (B, M) or tuple(image_hw.shape) != (B, 2) or area_ranges.dim() != 2 or area_ranges.shape[1] != 2:
        raise _lib.BdetrError(f"{what}: operand shapes disagree (gt_crowd [B,M], image_hw [B,2], area_ranges [A,2])")
    A = int(area_ranges.shape[0])
    if gt_count.numel() != A * num_classes:
        raise _lib.BdetrError(f"{what}: gt_count must be [A,C]")
    _chk(gt_crowd, dtype=torch.uint8)
    _chk(image_hw, gt_count, dtype=torch.int32)
    _chk(area_ranges, dtype=torch.float64)
    return A


def det_match_coco(score, label, box_pred, gt_label, gt_box, gt_crowd, gt_area, num_objects, image_hw, area_ranges, thresholds,
                   num_classes: int, max_dets: int, gt_count):
    """COCOeval's matching of one batch with crowd regions and area ranges (include/bdetr.h, K16).  gt_crowd uint8 [B,M]; gt_area f32
    [B,M] in pixels or None; image_hw int32 [B,2]; area_ranges float64 [A,2] in HBM; thresholds: host fp64 values; max_dets: the
    largest one; gt_count int32 [A,num_classes] in HBM, added to.  Returns (order int32 [B,N], class_rank int32 [B,N], tp_bits int16
    [A,B,N], ig_bits int16 [A,B,N] - uint16 bit patterns - and matched_gt int32 [A,B,T,N])."""
    _chk(score, box_pred, gt_box)
    _chk(label, gt_label, num_objects, dtype=torch.int32)
    B, N = score.shape
    M = gt_label.shape[1]
    if tuple(label.shape) != (B, N) or tuple(box_pred.shape) != (B, N, 4) or tuple(gt_label.shape) != (B, M) or tuple(gt_box.shape) != (B, M, 4) \
            or num_objects.numel() != B:
        raise _lib.BdetrError("det_match_coco: operand shapes disagree")
    A = _coco_operands("det_match_coco", B, M, gt_crowd, gt_area, image_hw, area_ranges, gt_count, int(num_classes))
    thr, T, order, class_rank, tp_bits, ig_bits, matched = _match_outputs(score, thresholds, A)
    check(_lib.lib().bdetr_det_match_coco(_p(score), _p(label), _p(box_pred), _p(gt_label), _p(gt_box), _p(gt_crowd), _p(gt_area), _p(num_objects),
                                          _p(image_hw), _p(area_ranges), thr.ctypes.data, B, N, M, int(num_classes), T, A, int(max_dets),
                                          _p(order), _p(class_rank), _p(tp_bits), _p(ig_bits), _p(matched), _p(gt_count), _stream()),
          "det_match_coco")
    return order, class_rank, tp_bits, ig_bits, matched


def mask_match_coco(score, label, det_bits, det_pop, gt_label, gt_bits, gt_pop, gt_crowd, gt_area, num_objects, image_hw, area_ranges,
                    thresholds, num_pixels: int, num_classes: int, max_dets: int, gt_count):
    """det_match_coco with packed masks in place of the boxes (include/bdetr.h, K17): det_bits / det_pop and gt_bits / gt_pop as
    mask_binarize returns them, num_pixels the masks' pixel count P.  Everything else, and what is returned, as det_match_coco."""
    _dtypes("mask_match_coco", score=(score, torch.float32), label=(label, torch.int32), det_bits=(det_bits, torch.int64),
            det_pop=(det_pop, torch.int32), gt_label=(gt_label, torch.int32), gt_bits=(gt_bits, torch.int64), gt_pop=(gt_pop, torch.int32),
            num_objects=(num_objects, torch.int32))
    if score.dim() != 2 or gt_label.dim() != 2 or det_bits.dim() != 3:
        raise _lib.BdetrError("mask_match_coco: operand shapes disagree (score [B,N], gt_label [B,M], det_bits [B,N,W])")
    B, N = score.shape
    M, W = gt_label.shape[1], det_bits.shape[2]
    P = int(num_pixels)
    if tuple(label.shape) != (B, N) or tuple(det_bits.shape) != (B, N, W) or tuple(det_pop.shape) != (B, N) or tuple(gt_label.shape) != (B, M) \
            or tuple(gt_bits.shape) != (B, M, W) or tuple(gt_pop.shape) != (B, M) or num_objects.numel() != B or W != (P + 63) // 64:
        raise _lib.BdetrError("mask_match_coco: operand shapes disagree")
    A = _coco_operands("mask_match_coco", B, M, gt_crowd, gt_area, image_hw, area_ranges, gt_count, int(num_classes))
    _chk(score)
    _chk(label, det_pop, gt_label, gt_pop, num_objects, dtype=torch.int32)
    _chk(det_bits, gt_bits, dtype=torch.int64)
    thr, T, order, class_rank, tp_bits, ig_bits, matched = _match_outputs(score, thresholds, A)
    check(_lib.lib().bdetr_mask_match_coco(_p(score), _p(label), _p(det_bits), _p(det_pop), _p(gt_label), _p(gt_bits), _p(gt_pop), _p(gt_crowd),
                                           _p(gt_area), _p(num_objects), _p(image_hw), _p(area_ranges), thr.ctypes.data, B, N, M, P,
                                           int(num_classes), T, A, int(max_dets), _p(order), _p(class_rank), _p(tp_bits), _p(ig_bits),
                                           _p(matched), _p(gt_count), _stream()), "mask_match_coco")
    return order, class_rank, tp_bits, ig_bits, matched


# --------------------------------------------------------------------------------------
# attribute-aware AP - csrc/attrmetric.hip (K29-K31)
# --------------------------------------------------------------------------------------
ATTR_MAX, ATTR_MAX_F1_THRESHOLDS, MATCH_LDS_LIMIT = 4096, 16, 64 * 1024


def attr_words(num_attributes: int) -> int:
    """Wa, the 64-bit words of an attribute set; a ValueError outside K29's limits (3 <= A <= 4096)."""
    A = int(num_attributes)
    if not 3 <= A <= ATTR_MAX:
        raise ValueError(f"attr_pack: num_attributes counts <PAD> and <OOV> and must be in [3, {ATTR_MAX}], got {A}")
    return (A + 63) // 64


def attr_match_lds_bytes(N: int, M: int, Wa: int, mask_words: Optional[int] = None) -> int:
    """The dynamic LDS a workgroup of K30 (mask_words None) or K31 (mask_words = W) needs: include/bdetr.h's formulas."""
    Np, Mp = (int(N) + 3) & ~3, (int(M) + 3) & ~3
    own = 36 * Np + 20 * Mp if mask_words is None else 24 * Np + 8 * Mp + 8 * int(mask_words) * (Np + Mp)
    return own + ((Np + Mp + 7) & ~7) + (8 * int(Wa) + 4) * (Np + Mp)


def check_attr_gate(what: str, N: int, M: int, Wa: int, f1_thresholds, empty_f1, mask_words: Optional[int] = None):
    """Every refusal of the gate that needs no device, as ValueError: F in [1, 16], empty_f1 0 or 1, Wa in [1, 64] and the staging
    within 64 KiB.  Returns (f1 thresholds as contiguous fp64, F, empty_f1 as float)."""
    f1 = np.ascontiguousarray(f1_thresholds, np.float64).reshape(-1)
    if not 1 <= f1.size <= ATTR_MAX_F1_THRESHOLDS:
        raise ValueError(f"{what}: 1 to {ATTR_MAX_F1_THRESHOLDS} F1 thresholds, got {f1.size}")
    if float(empty_f1) not in (0.0, 1.0):
        raise ValueError(f"{what}: empty_f1 is the F1 of two empty attribute sets, 0.0 or 1.0, got {empty_f1}")
    if not 1 <= int(Wa) <= ATTR_MAX // 64:
        raise ValueError(f"{what}: attribute sets have 1 to {ATTR_MAX // 64} words, got {Wa}")
    need = attr_match_lds_bytes(N, M, Wa, mask_words)
    if need > MATCH_LDS_LIMIT:
        raise ValueError(f"{what}: N={N} M={M} Wa={Wa}" + ("" if mask_words is None else f" W={mask_words}") + f" need {need} bytes of LDS per "
                         f"image, {(8 * int(Wa) + 4) * (((N + 3) & ~3) + ((M + 3) & ~3))} of them the attribute sets; the limit is {MATCH_LDS_LIMIT}")
    return f1, int(f1.size), float(empty_f1)


def attr_pack(x):
    """x [..., A] fp32 (attribute probabilities, or the tokenizer's multi-hot targets) -> (bits int64 [..., ceil(A/64)], count int32
    [...]) (include/bdetr.h, K29): bit a mod 64 of word a div 64 is a >= 2 and x[a] >= 0.5 (the reference's decode rule; NaN: false;
    <PAD> and <OOV> are never an attribute), the tail word's unused bits are zero, count = the row's set bits.  int64 holds the
    uint64 bit pattern."""
    _dtypes("attr_pack", x=(x, torch.float32))
    if x.dim() < 1 or x.numel() == 0:
        raise _lib.BdetrError(f"attr_pack: x must be [..., A] with at least one element, got {tuple(x.shape)}")
    A = x.shape[-1]
    Wa = attr_words(A)
    _chk(x)
    lead = tuple(x.shape[:-1])
    bits = empty(*lead, Wa, like=x, dtype=torch.int64)
    count = empty(*lead, like=x, dtype=torch.int32)
    check(_lib.lib().bdetr_attr_pack(_p(x), x.numel() // A, A, _p(bits), _p(count), _stream()), "attr_pack")
    return bits, count


def _attr_operands(what: str, B: int, N: int, M: int, det_attr, det_count, gt_attr, gt_attr_count) -> int:
    """The gate's operands, checked; returns Wa."""
    _dtypes(what, det_attr=(det_attr, torch.int64), det_count=(det_count, torch.int32), gt_attr=(gt_attr, torch.int64),
            gt_attr_count=(gt_attr_count, torch.int32))
    if det_attr.dim() != 3:
        raise _lib.BdetrError(f"{what}: det_attr must be [B,N,Wa]")
    Wa = int(det_attr.shape[2])
    if tuple(det_attr.shape) != (B, N, Wa) or tuple(det_count.shape) != (B, N) or tuple(gt_attr.shape) != (B, M, Wa) \
            or tuple(gt_attr_count.shape) != (B, M):
        raise _lib.BdetrError(f"{what}: operand shapes disagree (det_attr [B,N,Wa], det_count [B,N], gt_attr [B,M,Wa], gt_attr_count [B,M])")
    return Wa


def _match_outputs_attr(score, thresholds, A: int, F: int):
    """_match_outputs with the leading F of the gated kernels: tp_bits / ig_bits [F,A,B,N], matched_gt [F,A,B,T,N]."""
    B, N = score.shape
    thr = np.ascontiguousarray(thresholds, np.float64).reshape(-1)
    T = int(thr.size)
    order = empty(B, N, like=score, dtype=torch.int32)
    class_rank = empty(B, N, like=score, dtype=torch.int32)
    tp_bits = empty(F, max(A, 1), B, N, like=score, dtype=torch.int16)
    ig_bits = empty(F, max(A, 1), B, N, like=score, dtype=torch.int16)
    matched = empty(F, max(A, 1), B, max(T, 1), N, like=score, dtype=torch.int32)
    return thr, T, order, class_rank, tp_bits, ig_bits, matched


def det_match_attr(score, label, box_pred, det_attr, det_count, gt_label, gt_box, gt_attr, gt_attr_count, gt_crowd, gt_area, num_objects,
                   image_hw, area_ranges, thresholds, f1_thresholds, empty_f1, num_classes: int, max_dets: int, gt_count):
    """det_match_coco with the attribute F1 gate (include/bdetr.h, K30): det_attr int64 [B,N,Wa] / det_count int32 [B,N] and gt_attr
    int64 [B,M,Wa] / gt_attr_count int32 [B,M] as attr_pack returns them; f1_thresholds: host fp64 values (F of them); empty_f1: the
    F1 of two empty sets, 0.0 or 1.0.  Everything else as det_match_coco.  Returns (order int32 [B,N], class_rank int32 [B,N], tp_bits
    int16 [F,A,B,N], ig_bits int16 [F,A,B,N] - uint16 bit patterns - and matched_gt int32 [F,A,B,T,N]).  A gate outside the limits
    (F, empty_f1, Wa, the LDS staging) is a ValueError before anything is launched."""
    if score.dim() != 2 or gt_label.dim() != 2 or det_attr.dim() != 3:
        raise _lib.BdetrError("det_match_attr: operand shapes disagree (score [B,N], gt_label [B,M], det_attr [B,N,Wa])")
    B, N = score.shape
    M = gt_label.shape[1]
    f1, F, empty_f1 = check_attr_gate("det_match_attr", N, M, det_attr.shape[2], f1_thresholds, empty_f1)
    Wa = _attr_operands("det_match_attr", B, N, M, det_attr, det_count, gt_attr, gt_attr_count)
    _chk(score, box_pred, gt_box)
    _chk(label, gt_label, num_objects, det_count, gt_attr_count, dtype=torch.int32)
    _chk(det_attr, gt_attr, dtype=torch.int64)
    if tuple(label.shape) != (B, N) or tuple(box_pred.shape) != (B, N, 4) or tuple(gt_label.shape) != (B, M) or tuple(gt_box.shape) != (B, M, 4) \
            or num_objects.numel() != B:
        raise _lib.BdetrError("det_match_attr: operand shapes disagree")
    A = _coco_operands("det_match_attr", B, M, gt_crowd, gt_area, image_hw, area_ranges, gt_count, int(num_classes))
    thr, T, order, class_rank, tp_bits, ig_bits, matched = _match_outputs_attr(score, thresholds, A, F)
    check(_lib.lib().bdetr_det_match_attr(_p(score), _p(label), _p(box_pred), _p(det_attr), _p(det_count), _p(gt_label), _p(gt_box), _p(gt_attr),
                                          _p(gt_attr_count), _p(gt_crowd), _p(gt_area), _p(num_objects), _p(image_hw), _p(area_ranges),
                                          thr.ctypes.data, f1.ctypes.data, empty_f1, B, N, M, int(num_classes), Wa, T, F, A, int(max_dets),
                                          _p(order), _p(class_rank), _p(tp_bits), _p(ig_bits), _p(matched), _p(gt_count), _stream()),
          "det_match_attr")
    return order, class_rank, tp_bits, ig_bits, matched


def mask_match_attr(score, label, det_bits, det_pop, det_attr, det_count, gt_label, gt_bits, gt_pop, gt_attr, gt_attr_count, gt_crowd, gt_area,
                    num_objects, image_hw, area_ranges, thresholds, f1_thresholds, empty_f1, num_pixels: int, num_classes: int, max_dets: int,
                    gt_count):
    """mask_match_coco with the attribute F1 gate (include/bdetr.h, K31): the gate's operands and what is returned as det_match_attr,
    everything else as mask_match_coco."""
    _dtypes("mask_match_attr", score=(score, torch.float32), label=(label, torch.int32), det_bits=(det_bits, torch.int64),
            det_pop=(det_pop, torch.int32), gt_label=(gt_label, torch.int32), gt_bits=(gt_bits, torch.int64), gt_pop=(gt_pop, torch.int32),
            num_objects=(num_objects, torch.int32))
    if score.dim() != 2 or gt_label.dim() != 2 or det_bits.dim() != 3 or getattr(det_attr, "dim", lambda: 0)() != 3:
        raise _lib.BdetrError("mask_match_attr: operand shapes disagree (score [B,N], gt_label [B,M], det_bits [B,N,W], det_attr [B,N,Wa])")
    B, N = score.shape
    M, W = gt_label.shape[1], det_bits.shape[2]
    P = int(num_pixels)
    f1, F, empty_f1 = check_attr_gate("mask_match_attr", N, M, det_attr.shape[2], f1_thresholds, empty_f1, mask_words=W)
    Wa = _attr_operands("mask_match_attr", B, N, M, det_attr, det_count, gt_attr, gt_attr_count)
    if tuple(label.shape) != (B, N) or tuple(det_bits.shape) != (B, N, W) or tuple(det_pop.shape) != (B, N) or tuple(gt_label.shape) != (B, M) \
            or tuple(gt_bits.shape) != (B, M, W) or tuple(gt_pop.shape) != (B, M) or num_objects.numel() != B or W != (P + 63) // 64:
        raise _lib.BdetrError("mask_match_attr: operand shapes disagree")
    A = _coco_operands("mask_match_attr", B, M, gt_crowd, gt_area, image_hw, area_ranges, gt_count, int(num_classes))
    _chk(score)
    _chk(label, det_pop, gt_label, gt_pop, num_objects, det_count, gt_attr_count, dtype=torch.int32)
    _chk(det_bits, gt_bits, det_attr, gt_attr, dtype=torch.int64)
    thr, T, order, class_rank, tp_bits, ig_bits, matched = _match_outputs_attr(score, thresholds, A, F)
    check(_lib.lib().bdetr_mask_match_attr(_p(score), _p(label), _p(det_bits), _p(det_pop), _p(det_attr), _p(det_count), _p(gt_label), _p(gt_bits),
                                           _p(gt_pop), _p(gt_attr), _p(gt_attr_count), _p(gt_crowd), _p(gt_area), _p(num_objects), _p(image_hw),
                                           _p(area_ranges), thr.ctypes.data, f1.ctypes.data, empty_f1, B, N, M, P, int(num_classes), Wa, T, F, A,
                                           int(max_dets), _p(order), _p(class_rank), _p(tp_bits), _p(ig_bits), _p(matched), _p(gt_count),
                                           _stream()), "mask_match_attr")
    return order, class_rank, tp_bits, ig_bits, matched


# --------------------------------------------------------------------------------------
# mask targets from COCO segmentations - csrc/maskraster.hip (K18)
# --------------------------------------------------------------------------------------
MASK_KIND_NONE, MASK_KIND_POLY, MASK_KIND_RLE = 0, 1, 2
MASK_MAX_DIM, MASK_MAX_COORD, MASK_MAX_GRID = 4096, 1 << 23, 32


def _flat_ranges(starts, lengths):
    """Indices of the concatenated ranges [starts[k], starts[k] + lengths[k]) and, per index, the range it belongs to."""
    owner = np.repeat(np.arange(starts.size), lengths)
    first = np.cumsum(lengths) - lengths
    return np.arange(int(lengths.sum())) - np.repeat(first - starts, lengths), owner


def check_mask_pack(items, item_off, kind, hw, placement, grid: int):
    """The host arrays of bdetr_mask_targets against every rule include/bdetr.h states for them (the kernel cannot report): dtypes
    and shapes raise BdetrError, broken offsets and limits ValueError.  Vectorised over the objects.  Returns (B, M)."""
    for name, a in (("items", items), ("item_off", item_off), ("kind", kind), ("hw", hw), ("placement", placement)):
        if not isinstance(a, np.ndarray) or a.dtype != np.int32:
            raise _lib.BdetrError(f"mask_targets: {name} must be an int32 NumPy array, got {getattr(a, 'dtype', type(a).__name__)}")
    if kind.ndim != 2 or kind.size == 0:
        raise _lib.BdetrError(f"mask_targets: kind must be [B,M] with at least one element, got {kind.shape}")
    B, M = kind.shape
    if items.ndim != 1 or item_off.shape != (B * M + 1,) or hw.shape != (B, M, 2) or placement.shape != (B, 6):
        raise _lib.BdetrError("mask_targets: operand shapes disagree (items [T], item_off [B M + 1], kind [B,M], hw [B,M,2], placement [B,6])")
    if not 1 <= int(grid) <= MASK_MAX_GRID:
        raise ValueError(f"mask_targets: grid must be in [1, {MASK_MAX_GRID}], got {grid}")
    off = item_off.astype(np.int64)
    if off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > items.size:
        raise ValueError("mask_targets: item_off must be non-decreasing and stay inside the item buffer")
    if ((kind < 0) | (kind > MASK_KIND_RLE)).any():
        raise ValueError("mask_targets: kind must be 0 (none), 1 (polygon) or 2 (RLE)")
    used = kind != MASK_KIND_NONE
    if used.any() and ((hw[used] < 1) | (hw[used] > MASK_MAX_DIM)).any():
        raise ValueError(f"mask_targets: source height and width must be in [1, {MASK_MAX_DIM}], got up to {int(hw[used].max())}")
    p = placement.astype(np.int64)
    if ((p[:, :2] < 1) | (p[:, :2] > MASK_MAX_DIM)).any() or (p[:, 2:4] < 1).any() or (p[:, 4:] < 0).any() \
            or (p[:, 4] + p[:, 2] > p[:, 0]).any() or (p[:, 5] + p[:, 3] > p[:, 1]).any():
        raise ValueError(f"mask_targets: placement (H, W, new_h, new_w, off_h, off_w) needs 1 <= H, W <= {MASK_MAX_DIM}, new >= 1, off >= 0 "
                         "and off + new <= canvas")
    flat_kind, size, it = kind.reshape(-1), np.diff(off), items.astype(np.int64)

    def fail(objects, what):
        raise ValueError(f"mask_targets: object {int(objects[0])}: {what}")

    poly = np.flatnonzero(flat_kind == MASK_KIND_POLY)
    if poly.size:
        start, n = off[poly], size[poly]
        if (n < 2).any():
            fail(poly[n < 2], "a polygon's items are R, R + 1 ring offsets and the vertices")
        R = it[start]
        short = (R < 0) | (2 + R > n)
        if short.any():
            fail(poly[short], "a polygon's items are R, R + 1 ring offsets and the vertices")
        idx, owner = _flat_ranges(start + 1, R + 1)
        ring = it[idx]
        down = np.flatnonzero((np.diff(ring) < 0) & (owner[1:] == owner[:-1]))
        wrong = (ring[np.cumsum(R + 1) - (R + 1)] != 0) | (n != 2 + R + 2 * it[start + 1 + R])
        if down.size or wrong.any():
            fail(poly[owner[down]] if down.size else poly[wrong], "ring offsets must start at 0, be non-decreasing and end at the vertex count")
        idx, owner = _flat_ranges(start + 2 + R, n - 2 - R)
        far = np.abs(it[idx]) > MASK_MAX_COORD
        if far.any():
            fail(poly[owner[far]], "snapped coordinates must stay within +-2^23 (1/256 pixel)")
    rle = np.flatnonzero(flat_kind == MASK_KIND_RLE)
    if rle.size:
        start, n = off[rle], size[rle]
        what = "one-runs must be (start, length) pairs, ascending, disjoint and inside h * w"
        if (n % 2).any():
            fail(rle[n % 2 > 0], what)
        idx, owner = _flat_ranges(start, n)
        runs, owner = it[idx].reshape(-1, 2), owner[::2]
        pixels = hw.reshape(-1, 2).astype(np.int64).prod(axis=1)[rle]
        end = runs.sum(axis=1)
        broken = (runs < 0).any(axis=1) | (end > pixels[owner])
        broken[1:] |= (runs[1:, 0] < end[:-1]) & (owner[1:] == owner[:-1])
        if broken.any():
            fail(rle[owner[broken]], what)
    return B, M


def mask_targets(items, item_off, kind, hw, placement, grid: int = 23, device=None):
    """COCO segmentations -> (masks f32 [B,M,grid,grid], area int32 [B,M]) in HBM (include/bdetr.h, K18).  The operands are the HOST
    int32 arrays pipeline.pad_annotations(with_masks=True) packs: they are checked here (check_mask_pack) before anything is
    launched, go to the device in one copy, and nothing is read back."""
    B, M = check_mask_pack(items, item_off, kind, hw, placement, grid)
    G = int(grid)
    parts = [item_off.reshape(-1), kind.reshape(-1), hw.reshape(-1), placement.reshape(-1), items]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    buf = torch.from_numpy(np.concatenate(parts)).to(dev)
    d_off, d_kind, d_hw, d_place, d_items = torch.split(buf, [int(a.size) for a in parts])
    masks = empty(B, M, G, G, like=buf)
    area = empty(B, M, like=buf, dtype=torch.int32)
    check(_lib.lib().bdetr_mask_targets(_p(d_items) if items.size else None, int(items.size), _p(d_off), _p(d_kind), _p(d_hw), _p(d_place),
                                        B, M, G, _p(masks), _p(area), _stream()), "mask_targets")
    return masks, area


# --------------------------------------------------------------------------------------
# masks at image resolution - csrc/maskimage.hip (K19-K22)
# --------------------------------------------------------------------------------------
MASK_MAX_WORDS_PER_ROW = MASK_MAX_DIM // 64


def mask_layout(image_hw):
    """(Hm, Wm) of the batch layout K19-K22 share, from the HOST int array image_hw [B,2]: Hm = max height, Wm = ceil(max width / 64).
    Heights and widths outside [1, 4096] are a ValueError."""
    hw = np.asarray(image_hw)
    if hw.ndim != 2 or hw.shape[1] != 2 or hw.shape[0] < 1 or not np.issubdtype(hw.dtype, np.integer):
        raise _lib.BdetrError(f"mask_layout: image_hw must be a host integer array [B,2], got {getattr(hw, 'dtype', None)} {hw.shape}")
    if int(hw.min()) < 1 or int(hw.max()) > MASK_MAX_DIM:
        raise ValueError(f"mask_layout: image heights and widths must be in [1, {MASK_MAX_DIM}], got {int(hw.min())} .. {int(hw.max())}")
    return int(hw[:, 0].max()), (int(hw[:, 1].max()) + 63) // 64


def _check_layout(what: str, Hm: int, Wm: int):
    if not (1 <= int(Hm) <= MASK_MAX_DIM and 1 <= int(Wm) <= MASK_MAX_WORDS_PER_ROW):
        raise ValueError(f"{what}: the mask layout needs 1 <= Hm <= {MASK_MAX_DIM} and 1 <= Wm <= {MASK_MAX_WORDS_PER_ROW}, got Hm={Hm} Wm={Wm}")
    return int(Hm), int(Wm)


def mask_upsample_bits(logits, image_hw, Hm: int, Wm: int, out=None):
    """logits f32 [B,N,G,G], image_hw int32 [B,2] in HBM -> (bits int64 [B,N,Hm,Wm], pop int32 [B,N]) (include/bdetr.h, K19): every
    query's logits brought to its image's h_b x w_b by the fp64 bilinear rule stated there and cut at 0, packed 64 pixels of a row
    to a word.  Bits at x >= w_b and rows y >= h_b are written as zero.  out: a bits buffer to write into."""
    _dtypes("mask_upsample_bits", logits=(logits, torch.float32), image_hw=(image_hw, torch.int32))
    if logits.dim() != 4 or logits.shape[2] != logits.shape[3] or logits.numel() == 0:
        raise _lib.BdetrError(f"mask_upsample_bits: logits must be [B,N,G,G] with at least one element, got {tuple(logits.shape)}")
    B, N, G, _ = logits.shape
    if tuple(image_hw.shape) != (B, 2):
        raise _lib.BdetrError("mask_upsample_bits: operand shapes disagree (logits [B,N,G,G], image_hw [B,2])")
    if not 1 <= G <= MASK_MAX_GRID:
        raise ValueError(f"mask_upsample_bits: G must be in [1, {MASK_MAX_GRID}], got {G}")
    Hm, Wm = _check_layout("mask_upsample_bits", Hm, Wm)
    _chk(logits)
    _chk(image_hw, dtype=torch.int32)
    if out is None:
        out = empty(B, N, Hm, Wm, like=logits, dtype=torch.int64)
    else:
        _dtypes("mask_upsample_bits", out=(out, torch.int64))
        if tuple(out.shape) != (B, N, Hm, Wm):
            raise _lib.BdetrError("mask_upsample_bits: out must be [B,N,Hm,Wm]")
        _chk(out, dtype=torch.int64)
    pop = empty(B, N, like=logits, dtype=torch.int32)
    check(_lib.lib().bdetr_mask_upsample_bits(_p(logits), _p(image_hw), B, N, G, Hm, Wm, _p(out), _p(pop), _stream()), "mask_upsample_bits")
    return out, pop


def check_source_pack(items, item_off, kind, hw, Hm: int, Wm: int):
    """check_mask_pack for K20: the same rules for the host arrays (no placement), and every segmented object must fit the layout
    (h <= Hm, ceil(w / 64) <= Wm).  Returns (B, M)."""
    if not isinstance(kind, np.ndarray) or kind.ndim != 2:
        raise _lib.BdetrError(f"mask_source_bits: kind must be an int32 NumPy array [B,M], got {getattr(kind, 'shape', type(kind).__name__)}")
    B, M = check_mask_pack(items, item_off, kind, hw, np.tile(np.asarray([[1, 1, 1, 1, 0, 0]], np.int32), (kind.shape[0], 1)), 1)
    Hm, Wm = _check_layout("mask_source_bits", Hm, Wm)
    used = kind != MASK_KIND_NONE
    if used.any() and ((hw[..., 0][used] > Hm).any() or (hw[..., 1][used] > 64 * Wm).any()):
        raise ValueError(f"mask_source_bits: a segmented object's (h, w) does not fit the layout Hm={Hm}, Wm={Wm}")
    return B, M


def mask_source_bits(items, item_off, kind, hw, Hm: int, Wm: int, device=None, out=None):
    """The segments pack of pipeline.pad_annotations(with_masks=True) -> (bits int64 [B,M,Hm,Wm], pop int32 [B,M]) in HBM
    (include/bdetr.h, K20): every object's exact source mask by K18's rule, in the layout of mask_upsample_bits; pop is
    mask_targets' area.  The operands are HOST int32 arrays, checked here before anything is launched; one copy to the device,
    nothing read back.  out: a bits buffer to write into."""
    B, M = check_source_pack(items, item_off, kind, hw, Hm, Wm)
    Hm, Wm = int(Hm), int(Wm)
    parts = [item_off.reshape(-1), kind.reshape(-1), hw.reshape(-1), items]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    buf = torch.from_numpy(np.concatenate(parts)).to(dev)
    d_off, d_kind, d_hw, d_items = torch.split(buf, [int(a.size) for a in parts])
    if out is None:
        out = empty(B, M, Hm, Wm, like=buf, dtype=torch.int64)
    else:
        _dtypes("mask_source_bits", out=(out, torch.int64))
        if tuple(out.shape) != (B, M, Hm, Wm):
            raise _lib.BdetrError("mask_source_bits: out must be [B,M,Hm,Wm]")
        _chk(out, dtype=torch.int64)
    pop = empty(B, M, like=buf, dtype=torch.int32)
    check(_lib.lib().bdetr_mask_source_bits(_p(d_items) if items.size else None, int(items.size), _p(d_off), _p(d_kind), _p(d_hw), B, M, Hm, Wm,
                                            _p(out), _p(pop), _stream()), "mask_source_bits")
    return out, pop


def mask_inter(det_bits, gt_bits, num_objects):
    """det_bits int64 [B,N,Hm,Wm], gt_bits int64 [B,M,Hm,Wm], num_objects int32 [B] -> inter int32 [B,N,M] (include/bdetr.h, K21):
    the set bits two masks share, for the ground-truth rows m < num_objects[b]; 0 for the others.  Integer adds only."""
    _dtypes("mask_inter", det_bits=(det_bits, torch.int64), gt_bits=(gt_bits, torch.int64), num_objects=(num_objects, torch.int32))
    if det_bits.dim() != 4 or gt_bits.dim() != 4 or det_bits.numel() == 0 or gt_bits.numel() == 0:
        raise _lib.BdetrError("mask_inter: operand shapes disagree (det_bits [B,N,Hm,Wm], gt_bits [B,M,Hm,Wm])")
    B, N, Hm, Wm = det_bits.shape
    M = gt_bits.shape[1]
    if tuple(gt_bits.shape) != (B, M, Hm, Wm) or num_objects.numel() != B:
        raise _lib.BdetrError("mask_inter: operand shapes disagree (det_bits [B,N,Hm,Wm], gt_bits [B,M,Hm,Wm], num_objects [B])")
    _check_layout("mask_inter", Hm, Wm)
    _chk(det_bits, gt_bits, dtype=torch.int64)
    _chk(num_objects, dtype=torch.int32)
    inter = empty(B, N, M, like=det_bits, dtype=torch.int32)
    check(_lib.lib().bdetr_mask_inter(_p(det_bits), _p(gt_bits), _p(num_objects), B, N, M, Hm, Wm, _p(inter), _stream()), "mask_inter")
    return inter


def mask_match_coco_inter(score, label, inter, det_pop, gt_label, gt_pop, gt_crowd, gt_area, num_objects, image_hw, pix, area_ranges,
                          thresholds, num_classes: int, max_dets: int, gt_count):
    """mask_match_coco fed from an intersection instead of the bits (include/bdetr.h, K22): inter int32 [B,N,M] as mask_inter
    returns it, det_pop int32 [B,N] / gt_pop int32 [B,M] the masks' set bits, pix int32 [B] the pixels a mask of image b has.
    Everything else, and what is returned, as mask_match_coco."""
    _dtypes("mask_match_coco_inter", score=(score, torch.float32), label=(label, torch.int32), inter=(inter, torch.int32),
            det_pop=(det_pop, torch.int32), gt_label=(gt_label, torch.int32), gt_pop=(gt_pop, torch.int32), num_objects=(num_objects, torch.int32),
            pix=(pix, torch.int32))
    if score.dim() != 2 or gt_label.dim() != 2:
        raise _lib.BdetrError("mask_match_coco_inter: operand shapes disagree (score [B,N], gt_label [B,M], inter [B,N,M])")
    B, N = score.shape
    M = gt_label.shape[1]
    if tuple(label.shape) != (B, N) or tuple(inter.shape) != (B, N, M) or tuple(det_pop.shape) != (B, N) or tuple(gt_pop.shape) != (B, M) \
            or num_objects.numel() != B or pix.numel() != B:
        raise _lib.BdetrError("mask_match_coco_inter: operand shapes disagree (score [B,N], gt_label [B,M], inter [B,N,M], pix [B])")
    A = _coco_operands("mask_match_coco_inter", B, M, gt_crowd, gt_area, image_hw, area_ranges, gt_count, int(num_classes))
    _chk(score)
    _chk(label, inter, det_pop, gt_label, gt_pop, num_objects, pix, dtype=torch.int32)
    thr, T, order, class_rank, tp_bits, ig_bits, matched = _match_outputs(score, thresholds, A)
    check(_lib.lib().bdetr_mask_match_coco_inter(_p(score), _p(label), _p(inter), _p(det_pop), _p(gt_label), _p(gt_pop), _p(gt_crowd), _p(gt_area),
                                                 _p(num_objects), _p(image_hw), _p(pix), _p(area_ranges), thr.ctypes.data, B, N, M,
                                                 int(num_classes), T, A, int(max_dets), _p(order), _p(class_rank), _p(tp_bits), _p(ig_bits),
                                                 _p(matched), _p(gt_count), _stream()), "mask_match_coco_inter")
    return order, class_rank, tp_bits, ig_bits, matched


# --------------------------------------------------------------------------------------
# COCO run-length encoding of bitmasks - csrc/maskrle.hip (K27, K28)
# --------------------------------------------------------------------------------------
def _rle_operands(what: str, bits, image_hw, keep):
    """The operands K27 and K28 share, checked; returns (B, N, Hm, Wm)."""
    _dtypes(what, bits=(bits, torch.int64), image_hw=(image_hw, torch.int32))
    if bits.dim() != 4 or bits.numel() == 0:
        raise _lib.BdetrError(f"{what}: bits must be [B,N,Hm,Wm] with at least one element, got {tuple(bits.shape)}")
    B, N, Hm, Wm = bits.shape
    if tuple(image_hw.shape) != (B, 2):
        raise _lib.BdetrError(f"{what}: operand shapes disagree (bits [B,N,Hm,Wm], image_hw [B,2])")
    if keep is not None:
        _dtypes(what, keep=(keep, torch.uint8))
        if tuple(keep.shape) != (B, N):
            raise _lib.BdetrError(f"{what}: keep must be [B,N]")
        _chk(keep, dtype=torch.uint8)
    _check_layout(what, Hm, Wm)
    _chk(bits, dtype=torch.int64)
    _chk(image_hw, dtype=torch.int32)
    return B, N, Hm, Wm


def _mask_rle_count(what: str, bits, image_hw, keep):
    B, N, Hm, Wm = _rle_operands(what, bits, image_hw, keep)
    n_counts = empty(B, N, like=bits, dtype=torch.int32)
    check(_lib.lib().bdetr_mask_rle_count(_p(bits), _p(image_hw), _p(keep), B, N, Hm, Wm, _p(n_counts), _stream()), "mask_rle_count")
    return n_counts


def mask_rle_count(bits, image_hw, keep=None):
    """bits int64 [B,N,Hm,Wm] (mask_upsample_bits / panoptic_merge), image_hw int32 [B,2], keep uint8 [B,N] or None in HBM ->
    n_counts int32 [B,N] (include/bdetr.h, K27): the number of run lengths COCO's rleEncode gives every kept mask - its transitions
    in column-major order plus one -, 0 for a mask with keep == 0.  For callers that only size buffers; nothing is read back."""
    return _mask_rle_count("mask_rle_count", bits, image_hw, keep)


def mask_rle_encode(bits, image_hw, keep=None, max_bytes: int = 1 << 30):
    """bits int64 [B,N,Hm,Wm], image_hw int32 [B,2], keep uint8 [B,N] or None in HBM -> (counts int32 [total], offset int64 [B N + 1]),
    both in HBM (include/bdetr.h, K27 / K28): COCO's rleEncode of every kept mask - the run lengths of its pixels in column-major
    order, zeros first -, mask o's at counts[offset[o] : offset[o+1]]; a mask with keep == 0 has an empty span.  Only the pixels
    inside the image are looked at.  K27, a prefix sum on the device, then the total is read back - the one small synchronising
    copy of this path - to size counts; 4 * total > max_bytes is a ValueError before K28 is launched."""
    n_counts = _mask_rle_count("mask_rle_encode", bits, image_hw, keep)
    B, N, Hm, Wm = bits.shape
    offset = torch.zeros(B * N + 1, dtype=torch.int64, device=bits.device)
    torch.cumsum(n_counts.reshape(-1), 0, dtype=torch.int64, out=offset[1:])
    total = int(offset[-1].item())
    if 4 * total > int(max_bytes):
        raise ValueError(f"mask_rle_encode: the run lengths of this batch need {4 * total} bytes (4 x {total} counts); max_bytes is {int(max_bytes)}")
    counts = empty(total, like=bits, dtype=torch.int32)
    check(_lib.lib().bdetr_mask_rle_encode(_p(bits), _p(image_hw), _p(keep), _p(offset), B, N, Hm, Wm, total, _p(counts) if total else None,
                                           _stream()), "mask_rle_encode")
    return counts, offset


# --------------------------------------------------------------------------------------
# panoptic merge and panoptic quality - csrc/panopticmerge.hip (K23-K26)
# --------------------------------------------------------------------------------------
PANOPTIC_MAX_ROWS = 1024          # queries / ground-truth rows per image


def panoptic_select(score, label, threshold: float, num_classes: int, is_stuff=None):
    """score f32 [B,N], label int32 [B,N] (det_postprocess), is_stuff uint8 [C] or None -> seg_of int32 [B,N] (include/bdetr.h,
    K23): -1 when not score > threshold, the lowest kept query of the same label for a stuff class, otherwise n itself."""
    _dtypes("panoptic_select", score=(score, torch.float32), label=(label, torch.int32))
    if score.dim() != 2 or score.numel() == 0 or tuple(label.shape) != tuple(score.shape):
        raise _lib.BdetrError("panoptic_select: operand shapes disagree (score [B,N], label [B,N])")
    B, N = score.shape
    if N > PANOPTIC_MAX_ROWS:
        raise ValueError(f"panoptic_select: N must be in [1, {PANOPTIC_MAX_ROWS}], got {N}")
    if not 0.0 <= float(threshold) < 1.0:
        raise ValueError(f"panoptic_select: threshold must be in [0, 1), got {threshold}")
    if is_stuff is not None:
        _dtypes("panoptic_select", is_stuff=(is_stuff, torch.uint8))
        if is_stuff.dim() != 1 or is_stuff.numel() != int(num_classes):
            raise _lib.BdetrError(f"panoptic_select: is_stuff must be [C={int(num_classes)}]")
        _chk(is_stuff, dtype=torch.uint8)
    _chk(score)
    _chk(label, dtype=torch.int32)
    seg_of = empty(B, N, like=score, dtype=torch.int32)
    check(_lib.lib().bdetr_panoptic_select(_p(score), _p(label), _p(is_stuff), B, N, int(num_classes), float(threshold), _p(seg_of), _stream()),
          "panoptic_select")
    return seg_of


def panoptic_merge(logits, seg_of, image_hw, Hm: int, Wm: int, with_bits: bool = True):
    """logits f32 [B,N,G,G], seg_of int32 [B,N], image_hw int32 [B,2] in HBM -> (ids int16 [B,Hm,64 Wm], bits int64 [B,N,Hm,Wm] or
    None, pop int32 [B,N]) (include/bdetr.h, K24): per pixel the kept query (seg_of >= 0) with the largest positive value of
    mask_upsample_bits' rule wins, ids holds its seg_of (-1: void or outside the image), bits[b,s] the pixels of id s - pairwise
    disjoint - and pop their counts.  with_bits=False passes NULL: the bitmasks are not written."""
    _dtypes("panoptic_merge", logits=(logits, torch.float32), seg_of=(seg_of, torch.int32), image_hw=(image_hw, torch.int32))
    if logits.dim() != 4 or logits.shape[2] != logits.shape[3] or logits.numel() == 0:
        raise _lib.BdetrError(f"panoptic_merge: logits must be [B,N,G,G] with at least one element, got {tuple(logits.shape)}")
    B, N, G, _ = logits.shape
    if tuple(seg_of.shape) != (B, N) or tuple(image_hw.shape) != (B, 2):
        raise _lib.BdetrError("panoptic_merge: operand shapes disagree (logits [B,N,G,G], seg_of [B,N], image_hw [B,2])")
    if not 1 <= G <= MASK_MAX_GRID:
        raise ValueError(f"panoptic_merge: G must be in [1, {MASK_MAX_GRID}], got {G}")
    if N > PANOPTIC_MAX_ROWS:
        raise ValueError(f"panoptic_merge: N must be in [1, {PANOPTIC_MAX_ROWS}], got {N}")
    Hm, Wm = _check_layout("panoptic_merge", Hm, Wm)
    _chk(logits)
    _chk(seg_of, image_hw, dtype=torch.int32)
    ids = empty(B, Hm, 64 * Wm, like=logits, dtype=torch.int16)
    bits = empty(B, N, Hm, Wm, like=logits, dtype=torch.int64) if with_bits else None
    pop = empty(B, N, like=logits, dtype=torch.int32)
    check(_lib.lib().bdetr_panoptic_merge(_p(logits), _p(seg_of), _p(image_hw), B, N, G, Hm, Wm, _p(ids), _p(bits), _p(pop), _stream()),
          "panoptic_merge")
    return ids, bits, pop


def panoptic_gt_exclusive(gt_bits, gt_label, num_objects, num_classes: int):
    """mask_source_bits' gt_bits int64 [B,M,Hm,Wm] IN PLACE -> the ground truth as a panoptic map (include/bdetr.h, K25): rows at
    or past num_objects and rows with a label outside [2, C) are zeroed, every other row loses the pixels an earlier row covers.
    Returns gt_pop int32 [B,M], the exclusive pixel counts."""
    _dtypes("panoptic_gt_exclusive", gt_bits=(gt_bits, torch.int64), gt_label=(gt_label, torch.int32), num_objects=(num_objects, torch.int32))
    if gt_bits.dim() != 4 or gt_bits.numel() == 0:
        raise _lib.BdetrError(f"panoptic_gt_exclusive: gt_bits must be [B,M,Hm,Wm], got {tuple(gt_bits.shape)}")
    B, M, Hm, Wm = gt_bits.shape
    if tuple(gt_label.shape) != (B, M) or num_objects.numel() != B:
        raise _lib.BdetrError("panoptic_gt_exclusive: operand shapes disagree (gt_bits [B,M,Hm,Wm], gt_label [B,M], num_objects [B])")
    if M > PANOPTIC_MAX_ROWS:
        raise ValueError(f"panoptic_gt_exclusive: M must be in [1, {PANOPTIC_MAX_ROWS}], got {M}")
    _check_layout("panoptic_gt_exclusive", Hm, Wm)
    _chk(gt_bits, dtype=torch.int64)
    _chk(gt_label, num_objects, dtype=torch.int32)
    gt_pop = empty(B, M, like=gt_bits, dtype=torch.int32)
    check(_lib.lib().bdetr_panoptic_gt_exclusive(_p(gt_bits), _p(gt_label), _p(num_objects), B, M, int(num_classes), Hm, Wm, _p(gt_pop),
                                                 _stream()), "panoptic_gt_exclusive")
    return gt_pop


def panoptic_match(inter, pred_pop, pred_label, seg_of, gt_pop, gt_label, gt_crowd, num_objects, num_classes: int, min_area: int):
    """panopticapi's matching in integers (include/bdetr.h, K26): inter int32 [B,N,M] (mask_inter on the two disjoint sets),
    pred_pop / pred_label / seg_of int32 [B,N], gt_pop / gt_label int32 [B,M], gt_crowd uint8 [B,M] or None, num_objects int32 [B]
    -> (gt_state [B,M], pred_state [B,N], match_inter [B,M], match_union [B,M]), all int32."""
    _dtypes("panoptic_match", inter=(inter, torch.int32), pred_pop=(pred_pop, torch.int32), pred_label=(pred_label, torch.int32),
            seg_of=(seg_of, torch.int32), gt_pop=(gt_pop, torch.int32), gt_label=(gt_label, torch.int32), num_objects=(num_objects, torch.int32))
    if inter.dim() != 3 or inter.numel() == 0:
        raise _lib.BdetrError(f"panoptic_match: inter must be [B,N,M], got {tuple(inter.shape)}")
    B, N, M = inter.shape
    if any(tuple(t.shape) != (B, N) for t in (pred_pop, pred_label, seg_of)) or any(tuple(t.shape) != (B, M) for t in (gt_pop, gt_label)) \
            or num_objects.numel() != B:
        raise _lib.BdetrError("panoptic_match: operand shapes disagree (inter [B,N,M], pred_* / seg_of [B,N], gt_* [B,M], num_objects [B])")
    if gt_crowd is not None:
        _dtypes("panoptic_match", gt_crowd=(gt_crowd, torch.uint8))
        if tuple(gt_crowd.shape) != (B, M):
            raise _lib.BdetrError("panoptic_match: gt_crowd must be [B,M]")
        _chk(gt_crowd, dtype=torch.uint8)
    if N > PANOPTIC_MAX_ROWS or M > PANOPTIC_MAX_ROWS:
        raise ValueError(f"panoptic_match: N and M must be in [1, {PANOPTIC_MAX_ROWS}], got N={N} M={M}")
    if int(min_area) < 0:
        raise ValueError(f"panoptic_match: min_area must not be negative, got {min_area}")
    _chk(inter, pred_pop, pred_label, seg_of, gt_pop, gt_label, num_objects, dtype=torch.int32)
    gt_state = empty(B, M, like=inter, dtype=torch.int32)
    pred_state = empty(B, N, like=inter, dtype=torch.int32)
    match_inter = empty(B, M, like=inter, dtype=torch.int32)
    match_union = empty(B, M, like=inter, dtype=torch.int32)
    check(_lib.lib().bdetr_panoptic_match(_p(inter), _p(pred_pop), _p(pred_label), _p(seg_of), _p(gt_pop), _p(gt_label), _p(gt_crowd),
                                          _p(num_objects), B, N, M, int(num_classes), int(min_area), _p(gt_state), _p(pred_state),
                                          _p(match_inter), _p(match_union), _stream()), "panoptic_match")
    return gt_state, pred_state, match_inter, match_union


# --------------------------------------------------------------------------------------
# panoptic head pieces (forward) - csrc/panoptic.hip
# --------------------------------------------------------------------------------------
def pad4(c: int) -> int:
    return (c + 3) // 4 * 4


def resize_bilinear(x, H: int, W: int):
    _chk(x)
    B, h, w, Cc = x.shape
    out = empty(B, H, W, Cc, like=x)
    check(_lib.lib().bdetr_resize_bilinear_nhwc(_p(x), B, h, w, Cc, _p(out), H, W, _stream()), "resize_bilinear")
    return out


def layernorm_act(x, C_true: int, gamma, beta, eps: float, slope: float = 1.0, ld_out: Optional[int] = None):
    """LayerNormalization over the first C_true channels of x [..., ld] (+ leaky ReLU with `slope`); output [..., ld_out], pad = 0."""
    _chk(x, gamma, beta)
    ld = x.shape[-1]
    ldo = pad4(C_true) if ld_out is None else ld_out
    out = empty(*x.shape[:-1], ldo, like=x)
    rows = x.numel() // ld
    check(_lib.lib().bdetr_layernorm_act_fwd(_p(x), rows, C_true, ld, _p(gamma), _p(beta), eps, slope, _p(out), ldo, _stream()), "layernorm_act")
    return out


def copy_cols(src, C_true: int, dst, col0: int, src_col0: int = 0):
    """dst[..., col0 + c] = src[..., src_col0 + c] for c < C_true (src_col0: the concatenation's backward slices a gradient apart)."""
    _chk(src, dst)
    rows = src.numel() // src.shape[-1]
    assert src_col0 + C_true <= src.shape[-1] and dst.numel() // dst.shape[-1] == rows
    check(_lib.lib().bdetr_copy_cols(_p(src) + 4 * src_col0, rows, C_true, src.shape[-1], _p(dst), dst.shape[-1], col0, _stream()), "copy_cols")
    return dst


def nhwc_to_nchw(x, C_true: int):
    _chk(x)
    B, H, W, ld = x.shape
    out = empty(B, C_true, H * W, like=x)
    check(_lib.lib().bdetr_nhwc_to_nchw(_p(x), B, H * W, C_true, ld, _p(out), _stream()), "nhwc_to_nchw")
    return out


# --------------------------------------------------------------------------------------
# panoptic head training - csrc/panoptic.hip (backward pieces, weight pack, mask loss)
# --------------------------------------------------------------------------------------
def layernorm_act_bwd(x, C_true: int, gamma, beta, eps: float, slope: float, dout, dgamma=None, dbeta=None):
    """Adjoint of ``layernorm_act(x, C_true, gamma, beta, eps, slope)``: dx shaped like x (padding columns 0), dgamma / dbeta [C_true]
    (written, not added)."""
    _chk(x, gamma, beta, dout, dgamma, dbeta)
    L = _lib.lib()
    ld, ldo = x.shape[-1], dout.shape[-1]
    rows = x.numel() // ld
    assert dout.numel() // ldo == rows, (x.shape, dout.shape)
    nblk = L.bdetr_layernorm_act_bwd_chunks(rows)
    parts = empty(2, nblk, C_true, like=x)
    dx = torch.empty_like(x)
    dgamma = empty(C_true, like=x) if dgamma is None else dgamma
    dbeta = empty(C_true, like=x) if dbeta is None else dbeta
    check(L.bdetr_layernorm_act_bwd(_p(x), rows, C_true, ld, _p(gamma), _p(beta), eps, slope, _p(dout), ldo, _p(dx), _p(parts[0]), _p(parts[1]),
                                    _p(dgamma), _p(dbeta), _stream()), "layernorm_act_bwd")
    return dx, dgamma, dbeta


def resize_bilinear_bwd(dout, h: int, w: int):
    """Adjoint of ``resize_bilinear(x [B,h,w,C], H, W)``."""
    _chk(dout)
    B, H, W, Cc = dout.shape
    din = empty(B, h, w, Cc, like=dout)
    check(_lib.lib().bdetr_resize_bilinear_nhwc_bwd(_p(dout), B, H, W, Cc, _p(din), h, w, _stream()), "resize_bilinear_bwd")
    return din


def nchw_to_nhwc(x, H: int, W: int, ld_out: int):
    """x [B, C, H*W] -> [B, H, W, ld_out] (columns C.. ld_out-1 zero): the adjoint of ``nhwc_to_nchw``."""
    _chk(x)
    B, Cc, P = x.shape
    assert P == H * W
    out = empty(B, H, W, ld_out, like=x)
    check(_lib.lib().bdetr_nchw_to_nhwc(_p(x), B, P, Cc, _p(out), ld_out, _stream()), "nchw_to_nhwc")
    return out


def conv_weight_pack(kernel, bias, transpose: bool):
    """Keras-layout kernel (HWIO [R,S,Cin,K]; transpose: Conv2DTranspose [R,S,K,Cin]) + bias [K] -> zero-padded OHWI
    [pad4(K), R, S, pad4(Cin)] (taps flipped for transpose) and bias [pad4(K)]."""
    _chk(kernel, bias)
    R, S = kernel.shape[0], kernel.shape[1]
    Kc, Cin = (kernel.shape[2], kernel.shape[3]) if transpose else (kernel.shape[3], kernel.shape[2])
    Kp, Cp = pad4(Kc), pad4(Cin)
    w = empty(Kp, R, S, Cp, like=kernel)
    b = empty(Kp, like=kernel)
    check(_lib.lib().bdetr_conv_weight_pack(_p(kernel), _p(bias), R, S, Cin, Kc, int(transpose), Cp, Kp, _p(w), _p(b), _stream()), "conv_weight_pack")
    return w, b


def conv_weight_unpack(dw, db, keras_shape, transpose: bool, dkernel=None, dbias=None):
    """Adjoint of ``conv_weight_pack``: the true-channel part of the padded dw / db into Keras-layout dkernel / dbias (either may be None)."""
    _chk(dw, db, dkernel, dbias)
    R, S = keras_shape[0], keras_shape[1]
    Kc, Cin = (keras_shape[2], keras_shape[3]) if transpose else (keras_shape[3], keras_shape[2])
    if dkernel is None and dbias is None:
        return None, None
    check(_lib.lib().bdetr_conv_weight_unpack(_p(dw), _p(db), R, S, Cin, Kc, int(transpose), dw.shape[-1], _p(dkernel), _p(dbias), _stream()),
          "conv_weight_unpack")
    return dkernel, dbias


MASK_FOCAL_ALPHA, MASK_FOCAL_GAMMA = 0.25, 2.0


def mask_loss(logits, masks, match, num_objects, mask_weight=1.0, loss_scale=1.0, want_grads=True):
    """logits [B,N,P], masks [B,M,P], match int32 [B,M], num_objects int32 [B] -> (loss [B], dlogits [B,N,P] | None)."""
    _chk(logits, masks)
    _chk(match, num_objects, dtype=torch.int32)
    B, N, P = logits.shape
    M = masks.shape[1]
    assert masks.shape == (B, M, P) and match.shape == (B, M), (logits.shape, masks.shape, match.shape)
    row_loss = empty(B, N, like=logits)
    loss = empty(B, like=logits)
    dlogits = torch.empty_like(logits) if want_grads else None
    check(_lib.lib().bdetr_mask_loss(_p(logits), _p(masks), _p(match), _p(num_objects), B, M, N, P, MASK_FOCAL_ALPHA, MASK_FOCAL_GAMMA,
                                     float(mask_weight), float(loss_scale), _p(row_loss), _p(loss), _p(dlogits), _stream()), "mask_loss")
    return loss, dlogits
