"""Plain-loop reference of the mask-target rule (include/bdetr.h, K18), in NumPy int64.  Imports nothing from the product.

Everything is integer up to the final fp64 division, so the GPU tests compare bit for bit.  The codec below is a scratch restatement
of the public COCO compressed-RLE description (pycocotools is not available here, so nothing in this file was produced with it).
"""
import numpy as np

DEFAULT_PLACEMENT = (1, 1, 1, 1, 0, 0)          # new = canvas, off = 0: the result depends only on h, w


def snap(ring):
    """flat [x0, y0, x1, y1, ...] in pixels -> int64 [V, 2] in 1/256 pixel (round half to even)."""
    v = np.asarray(ring, np.float64).reshape(-1, 2)
    return np.rint(v * 256.0).astype(np.int64)


def ring_mask(q, h, w):
    """One snapped ring -> bool [h, w] by the per-edge crossing test at every pixel centre (even-odd)."""
    count = np.zeros((h, w), np.int64)
    if len(q) < 3:
        return count.astype(bool)
    cx = (256 * np.arange(w, dtype=np.int64) + 128)[None, :]
    cy = (256 * np.arange(h, dtype=np.int64) + 128)[:, None]
    for k in range(len(q)):
        a, b = q[k], q[(k + 1) % len(q)]
        if a[1] == b[1]:
            continue
        lo, hi = (a, b) if a[1] < b[1] else (b, a)
        crosses = (a[1] <= cy) != (b[1] <= cy)
        left = (cy - lo[1]) * (hi[0] - lo[0]) <= (cx - lo[0]) * (hi[1] - lo[1])
        count += (crosses & left).astype(np.int64)
    return (count & 1).astype(bool)


def polygon_mask(rings, h, w):
    """Union (OR) over the rings."""
    m = np.zeros((h, w), bool)
    for ring in rings:
        m |= ring_mask(snap(ring), h, w)
    return m


def rle_mask(counts, h, w):
    """Runs alternate zeros and ones, start with zeros, column-major."""
    counts = [int(c) for c in counts]
    assert all(c >= 0 for c in counts) and sum(counts) == h * w
    flat = np.zeros(h * w, bool)
    p = 0
    for k, c in enumerate(counts):
        if k & 1:
            flat[p:p + c] = True
        p += c
    return flat.reshape(w, h).T.copy()


def mask_to_counts(mask):
    """bool [h, w] -> uncompressed COCO counts."""
    flat = np.asarray(mask, bool).T.reshape(-1)
    counts, cur, run = [], False, 0
    for v in flat:
        if v != cur:
            counts.append(run)
            cur, run = v, 0
        run += 1
    counts.append(run)
    return counts


def weights(n, G, canvas, new, off):
    """OY [n, G] int64 (rows y, cells i); the same formula gives OX."""
    y = np.arange(n, dtype=np.int64)[:, None]
    i = np.arange(G, dtype=np.int64)[None, :]
    p0 = G * (n * off + y * new)
    return np.maximum(0, np.minimum(p0 + G * new, (i + 1) * canvas * n) - np.maximum(p0, i * canvas * n))


def numerator(mask, G, placement=DEFAULT_PLACEMENT):
    H, W, new_h, new_w, off_h, off_w = (int(v) for v in placement)
    h, w = mask.shape
    return weights(h, G, H, new_h, off_h).T @ mask.astype(np.int64) @ weights(w, G, W, new_w, off_w)


def target(mask, G, placement=DEFAULT_PLACEMENT):
    """(masks f32 [G, G], area int)."""
    H, W = int(placement[0]), int(placement[1])
    h, w = mask.shape
    N = numerator(mask, G, placement)
    return (N.astype(np.float64) / np.float64(H * h * W * w)).astype(np.float32), int(mask.sum())


def segmentation_mask(seg, h, w):
    """A COCO segmentation (list of rings, RLE dict, or None) -> bool [h, w]."""
    if seg is None:
        return np.zeros((h, w), bool)
    if isinstance(seg, dict):
        counts = seg["counts"]
        if isinstance(counts, (str, bytes)):
            counts = decode(counts)
        return rle_mask(counts, h, w)
    return polygon_mask(seg, h, w)


# ---------------------------------------------------------------------------------------------------------------------
# the compressed-string codec, restated from the public format description
# ---------------------------------------------------------------------------------------------------------------------
def decode(s):
    if isinstance(s, str):
        s = s.encode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def encode(counts):
    out = []
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            c5 = x & 0x1F
            x >>= 5
            more = (x != -1) if (c5 & 0x10) else (x != 0)
            out.append(chr((c5 | (0x20 if more else 0)) + 48))
    return "".join(out)
