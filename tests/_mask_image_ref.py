"""Plain NumPy reference of the image-resolution mask path (include/bdetr.h, K19 and K21, and the layout K19-K22 share).  Imports
nothing from the product.  Source masks (K20) come from tests/_mask_raster_ref.py, matching and the summary (K22) from
tests/_coco_ref.py on the flattened h x w boolean masks.

The upsample rule is fp64 with every operation rounded on its own - what NumPy does with whole-array operations - so the GPU tests
compare bit for bit."""
import numpy as np


def axis_rule(n, G):
    """Per target pixel p of n along an axis of G source cells: (ia, ib int64 [n], t float64 [n])."""
    p = np.arange(n, dtype=np.int64)
    num = (2 * p + 1) * G - n
    D = 2 * n
    i0 = num // D                                   # floor division: -1 for a negative num
    r = num - i0 * D
    ia = np.maximum(i0, 0)
    ib = np.minimum(i0 + 1, G - 1)
    return ia, ib, r.astype(np.float64) / np.float64(D)


def upsample(logits, h, w):
    """logits [G, G] float32 -> the rule's value, float64 [h, w]."""
    L = np.asarray(logits, np.float32).astype(np.float64)
    G = L.shape[0]
    assert L.shape == (G, G)
    ya, yb, ty = axis_rule(h, G)
    xa, xb, tx = axis_rule(w, G)
    ux, uy = 1.0 - tx, 1.0 - ty
    with np.errstate(invalid="ignore", over="ignore"):
        top = ux[None, :] * L[ya][:, xa] + tx[None, :] * L[ya][:, xb]
        bot = ux[None, :] * L[yb][:, xa] + tx[None, :] * L[yb][:, xb]
        return uy[:, None] * top + ty[:, None] * bot


def upsample_mask(logits, h, w):
    """bool [h, w]: the value > 0 (NaN: False)."""
    with np.errstate(invalid="ignore"):
        return np.greater(upsample(logits, h, w), 0.0)


def layout(image_hw):
    hw = np.asarray(image_hw, np.int64).reshape(-1, 2)
    return int(hw[:, 0].max()), (int(hw[:, 1].max()) + 63) // 64


def pack(mask, Hm, Wm):
    """bool [h, w] -> uint64 [Hm, Wm]: pixel (x, y) is bit x mod 64 of word [y, x div 64]; everything else zero."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    assert h <= Hm and w <= 64 * Wm
    full = np.zeros((Hm, Wm * 64), np.uint64)
    full[:h, :w] = mask
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (full.reshape(Hm, Wm, 64) * weights).sum(axis=2, dtype=np.uint64)


def unpack(bits, h, w):
    """The inverse of pack on the image's own pixels: uint64 [Hm, Wm] -> bool [h, w]."""
    bits = np.asarray(bits).view(np.uint64)
    Hm, Wm = bits.shape
    full = ((bits[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(Hm, Wm * 64)
    return full[:h, :w].copy()


def popcount(words):
    w = np.ascontiguousarray(np.asarray(words).view(np.uint64))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1).sum(axis=(-1, -2)).astype(np.int64)


def inter(det_bits, gt_bits, num_objects):
    """det_bits [B,N,Hm,Wm], gt_bits [B,M,Hm,Wm] uint64, num_objects [B] -> int32 [B,N,M]; rows m >= num_objects are 0."""
    d, g = np.asarray(det_bits).view(np.uint64), np.asarray(gt_bits).view(np.uint64)
    B, N, M = d.shape[0], d.shape[1], g.shape[1]
    out = np.zeros((B, N, M), np.int32)
    for b in range(B):
        for m in range(max(0, min(int(num_objects[b]), M))):
            out[b, :, m] = popcount((d[b] & g[b, m][None]).reshape(N, -1))
    return out
