"""Plain-loop reference of COCO's rleEncode on the bitmask layout of K19-K28 (include/bdetr.h).  Imports nothing from the product.

The encoder walks the pixels one at a time, in column-major order, exactly as the rule is stated: no vectorised step that could
share a mistake with the kernels.  pack() is the only fast routine here; it builds test INPUTS (np.packbits), never expectations."""
import numpy as np


def unpack(bits, h, w):
    """uint64 (or int64) [Hm, Wm] -> bool [h, w]: pixel (x, y) is bit x mod 64 of word [y, x div 64]; everything outside is ignored."""
    words = np.asarray(bits).view(np.uint64)
    mask = np.zeros((h, w), bool)
    for y in range(h):
        row = [int(v) for v in words[y]]
        for x in range(w):
            mask[y, x] = (row[x >> 6] >> (x & 63)) & 1
    return mask


def rle_encode(mask):
    """bool [h, w] -> the list of run lengths: pixels in Fortran order, runs of 0 and 1 alternating, starting with a run of 0."""
    flat = np.asarray(mask, bool).flatten(order="F").tolist()
    counts, current, run = [], False, 0
    for pixel in flat:
        if pixel != current:
            counts.append(run)
            current, run = pixel, 0
        run += 1
    counts.append(run)
    return counts


def encode_bits(bits, h, w):
    return rle_encode(unpack(bits, h, w))


def encode_batch(bits, image_hw, keep=None):
    """bits [B,N,Hm,Wm], image_hw [B,2], keep [B,N] or None -> (counts int32 [total], offset int64 [B N + 1], the per-mask lists)."""
    bits = np.asarray(bits)
    B, N = bits.shape[:2]
    lists = []
    for b in range(B):
        h, w = (int(v) for v in image_hw[b])
        for n in range(N):
            lists.append(encode_bits(bits[b, n], h, w) if keep is None or keep[b][n] else [])
    offset = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    counts = np.asarray([v for c in lists for v in c], np.int32)
    return counts, offset, lists


def pack(mask, Hm, Wm, fill=None):
    """bool [h, w] -> uint64 [Hm, Wm] in the kernels' layout.  fill: uint64 [Hm, Wm] words whose bits are taken outside the image
    (garbage for the tests that prove the padding is not relied on); None: zeros."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    wpr = (w + 63) // 64
    assert 1 <= h <= Hm and 1 <= w and wpr <= Wm
    out = np.zeros((Hm, Wm), np.uint64) if fill is None else np.array(fill, np.uint64).reshape(Hm, Wm)
    rows = np.zeros((h, wpr * 64), bool)
    rows[:, :w] = mask
    words = np.packbits(rows, axis=1, bitorder="little").view(np.uint64).reshape(h, wpr)
    inside = np.packbits(np.arange(wpr * 64) < w, bitorder="little").view(np.uint64)          # per word column: the image's own bits
    out[:h, :wpr] = words | (out[:h, :wpr] & ~inside[None, :])
    return out


def counts_to_mask(counts, h, w):
    """The inverse of rle_encode, by a plain loop: run lengths -> bool [h, w]."""
    flat, value = [], False
    for c in counts:
        flat.extend([value] * int(c))
        value = not value
    assert len(flat) == h * w
    return np.asarray(flat, bool).reshape((h, w), order="F")
