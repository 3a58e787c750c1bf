"""Plain torch restatement of the backbone's residual units (boosted_detr_amd/backbone.py, ResNet.call's bottleneck loop) with autograd,
in fp64 - and, through `dtype=`, in fp32: the yardstick the stage-parity tolerances are derived from (tests/test_resunit_gpu.py).

Layouts are the project's: activations [N, H, W, C], convolution kernels [K, R, S, C].  A unit is a dict {"short": p | None, "c1": p,
"c2": p, "c3": p} like ResNet.blocks, every p = {"kernel", "bias", "gamma", "beta"}.

Every ReLU takes an optional `decisions` tensor (bool, the shape of its input): given, the ReLU is pre * decisions - the reference
then differentiates the function the DEVICE evaluated, and a pre-activation that rounds to the other side of zero there does not
show up as a gradient error; not given, it is pre * (pre > 0).

Also here: the host decoder / encoder of bn_apply_p16's ReLU bit-mask words (csrc/norm.hip: element e of float4 index i lives in
word (i >> 6) * 4 + e, bit i & 63).  Pure CPU: no kernel, no device."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1.001e-5                                               # backbone.RESNET_BN_EPS
STAGES = ((64, 3, 1), (128, 2, 2), (256, 1, 2))              # the miniature of the stage-parity tests: (filters, units, first stride)
POOL_HW = {"even": (8, 12), "odd": (9, 7)}                   # the stem's pooled map for prepared images of 32 x 48 and 34 x 26
LAYERS = ("short", "c1", "c2", "c3")


def relu(pre, decisions=None):
    keep = (pre > 0) if decisions is None else decisions
    return pre * keep.to(pre.dtype)


def batchnorm(y, gamma, beta):
    """Train-mode BatchNormalization over all but the last axis: biased variance of the tensor itself."""
    axes = tuple(range(y.dim() - 1))
    m = y.mean(axes)
    v = ((y - m) ** 2).mean(axes)
    return (y - m) / torch.sqrt(v + EPS) * gamma + beta


def conv_bn(x, p, stride, pad):
    """Conv2D with bias, then train-mode BatchNorm (no activation)."""
    y = F.conv2d(x.permute(0, 3, 1, 2), p["kernel"].permute(0, 3, 1, 2), p["bias"], stride=stride, padding=pad).permute(0, 2, 3, 1)
    return batchnorm(y, p["gamma"], p["beta"])


def unit(x, blk, stride, decisions=None, record=None, name="u"):
    """One bottleneck: the stride on the first 1x1, a projection shortcut where the unit has one, relu(bn(c3) + shortcut).
    decisions: {layer name: bool tensor} for the three ReLUs (missing names decide for themselves); record: a dict that receives
    every layer's pre-activation (name + '.pre') and output (name)."""
    d = decisions or {}
    rec = record if record is not None else {}
    sc = x
    if blk["short"] is not None:
        sc = rec[f"{name}.short"] = conv_bn(x, blk["short"], stride, 0)
    y = x
    for layer, s, pad in (("c1", stride, 0), ("c2", 1, 1), ("c3", 1, 0)):
        pre = conv_bn(y, blk[layer], s, pad)
        if layer == "c3":
            pre = pre + sc
        rec[f"{name}.{layer}.pre"] = pre
        y = rec[f"{name}.{layer}"] = relu(pre, d.get(f"{name}.{layer}"))
    return y


def unit_strides(stages):
    """(stage index, unit index in the stage, stride) of every unit, in order."""
    return [(si, bi, stride1 if bi == 0 else 1) for si, (_, n, stride1) in enumerate(stages) for bi in range(n)]


def unit_name(i):
    return f"u{i}"


def net(stages, x, blocks, decisions=None):
    """The block loop of ResNet.call from the pooled stem output `x` on: returns (output, record of every layer)."""
    rec = {}
    for i, (_, _, stride) in enumerate(unit_strides(stages)):
        x = unit(x, blocks[i], stride, decisions, rec, unit_name(i))
    return x, rec


def random_blocks(stages, seed, cin=64):
    """Host parameters of the topology: glorot-uniform kernels, biases / gamma / beta away from 0 / 1 (numpy fp32)."""
    rng = np.random.default_rng(seed)
    blocks = []

    def layer(c, k, r):
        lim = (6.0 / (r * r * (c + k))) ** 0.5
        return {"kernel": rng.uniform(-lim, lim, (k, r, r, c)).astype(np.float32), "bias": (0.2 * rng.standard_normal(k)).astype(np.float32),
                "gamma": (1 + 0.2 * rng.standard_normal(k)).astype(np.float32), "beta": (0.2 * rng.standard_normal(k)).astype(np.float32)}

    for f, n, _ in stages:
        for bi in range(n):
            blocks.append({"short": layer(cin, 4 * f, 1) if bi == 0 else None, "c1": layer(cin, f, 1), "c2": layer(f, f, 3), "c3": layer(f, 4 * f, 1)})
            cin = 4 * f
    return blocks


def leaves(blocks, dtype=torch.float64):
    """The host parameters as autograd leaves of `dtype`."""
    def leaf(a):
        return torch.as_tensor(np.asarray(a)).to(dtype).clone().requires_grad_(True)
    return [{k: (None if p is None else {n: leaf(a) for n, a in p.items()}) for k, p in blk.items()} for blk in blocks]


def run(stages, x, blocks, dtype=torch.float64, decisions=None, gout=None):
    """One reference pass in `dtype` from host values: (record of detached layer tensors, {'u3.c1.kernel': gradient} | None)."""
    p = leaves(blocks, dtype)
    out, rec = net(stages, torch.as_tensor(x).to(dtype), p, decisions)
    grads = None
    if gout is not None:
        out.backward(torch.as_tensor(gout).to(dtype))
        grads = {f"{unit_name(i)}.{layer}.{n}": t.grad for i, blk in enumerate(p) for layer in LAYERS if blk[layer] is not None
                 for n, t in blk[layer].items()}
    return {k: v.detach() for k, v in rec.items()}, grads


def deviation(got, ref, floor=0.0):
    """max |got - ref| over the tensor's scale: max |ref|, and at least `floor`."""
    ref = ref.double()
    scale = max(float(ref.abs().max()), floor, 1e-300)
    return float((got.double() - ref).abs().max()) / scale


# ---- the ReLU bit mask of bn_apply_p16 ----
def mask_decode(words, numel):
    """int64 mask words -> bool [numel]: element e of float4 index i lives in word (i >> 6) * 4 + e, bit i & 63."""
    w = np.ascontiguousarray(torch.as_tensor(words).cpu().numpy()).view(np.uint64)
    assert numel % 4 == 0 and w.size >= ((numel // 4 + 63) // 64) * 4, (numel, w.size)
    i = np.arange(numel // 4, dtype=np.uint64)
    out = np.empty((numel // 4, 4), dtype=bool)
    for e in range(4):
        out[:, e] = (w[(i >> np.uint64(6)) * np.uint64(4) + np.uint64(e)] >> (i & np.uint64(63))) & np.uint64(1)
    return torch.from_numpy(out.reshape(-1))


def mask_encode(keep):
    """bool [numel] -> the int64 words bn_apply_p16 writes for it (the bits of a partial last group past the tensor's end are zero)."""
    keep = np.asarray(torch.as_tensor(keep).cpu().numpy(), dtype=bool).reshape(-1, 4)
    n4 = keep.shape[0]
    w = np.zeros(((n4 + 63) // 64) * 4, dtype=np.uint64)
    for i in range(n4):
        for e in range(4):
            if keep[i, e]:
                w[(i >> 6) * 4 + e] |= np.uint64(1) << np.uint64(i & 63)
    return torch.from_numpy(w.view(np.int64).copy())
