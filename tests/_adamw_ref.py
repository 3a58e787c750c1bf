"""Restatements of the AdamW update (boosted_detr_amd.training.AdamW, include/bdetr.h K13) for the tests, and the seeded synthetic
tensors the optimizer kernel tests run on.

AdamW = Keras Adam (non-amsgrad) + TFA's DecoupledWeightDecayExtension + Keras' per-tensor clipnorm.  For step t = iterations + 1:

    g   <- g * grad_scale ;  g <- g * min(1, clipnorm / ||g||_2)      (clipnorm 0 = off)
    w   <- w - wd_t * w                                               (decoupled: NOT multiplied by lr; skipped for excluded tensors)
    m   <- b1*m + (1-b1)*g ;  v <- b2*v + (1-b2)*g*g
    lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)
    w   <- w - lr_t * m / (sqrt(v) + eps)

``adamw_step64`` is that in float64 (pinned to torch.optim.AdamW by tests/test_adamw_cpu.py); ``adamw_step32`` is the same in NumPy
float32 in the op order the header documents, every operation rounded on its own, fed the fp32 scalars the host stages.
"""
import math

import numpy as np

DEFAULTS = dict(b1=0.9, b2=0.999, eps=1e-7)


def lr_t64(lr: float, t: int, b1: float, b2: float) -> float:
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def adamw_step64(w, g, m, v, *, lr, wd, t, b1=0.9, b2=0.999, eps=1e-7, clipnorm=0.0, grad_scale=1.0, decay=True):
    """One step in float64 from (w, m, v) and the gradient g; returns the new (w, m, v)."""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    g = g * grad_scale
    if clipnorm and clipnorm > 0:
        nrm = math.sqrt(float((g * g).sum()))
        if nrm > clipnorm:
            g = g * (clipnorm / nrm)
    if decay:
        w = w - wd * w
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    w = w - lr_t64(lr, t, b1, b2) * m / (np.sqrt(v) + eps)
    return w, m, v


SLAB = 16384          # bdetr_sgd_slab_elems()


def norm32(g) -> np.float32:
    g = np.asarray(g, np.float32)
    parts = [np.sum(g[o: o + SLAB] * g[o: o + SLAB], dtype=np.float32) for o in range(0, g.size, SLAB)]
    return np.float32(math.sqrt(float(np.sum(np.asarray(parts, np.float64)))))


def adamw_step32(w, g, m, v, *, lr, wd, t, b1=0.9, b2=0.999, eps=1e-7, clipnorm=0.0, grad_scale=1.0, decay=True):
    """The kernel's arithmetic in NumPy float32: the scalars are what the host hands the kernel (lr_t, 1-b1, 1-b2 computed in double and
    rounded once), every product, sum, square root and quotient is rounded to fp32 on its own.  The gradient norm as the header
    documents it: fp32 squares summed in fp32 within a slab of 16,384 elements (NumPy's order of additions inside a slab is not the
    kernel's - both are fp32 sums), the slabs' sums added in double, square root in double, rounded once to fp32."""
    f = np.float32
    w, g, m, v = (np.asarray(a, f) for a in (w, g, m, v))
    lr_t, wd_t = f(lr_t64(lr, t, b1, b2)), f(wd)
    c1, c2, o1, o2, e = f(b1), f(b2), f(1.0 - b1), f(1.0 - b2), f(eps)
    scale = f(grad_scale)
    if clipnorm and clipnorm > 0:
        nrm = f(norm32(g) * f(abs(grad_scale)))
        if nrm > f(clipnorm):
            scale = f(scale * f(f(clipnorm) / nrm))
    gi = g * scale
    w1 = w - wd_t * w if decay else w
    mn = c1 * m + o1 * gi
    vn = c2 * v + o2 * (gi * gi)
    wn = w1 - (lr_t * mn) / (np.sqrt(vn) + e)
    assert wn.dtype == mn.dtype == vn.dtype == np.float32
    return wn, mn, vn


def sgd_step64(w, g, v, *, lr, momentum=0.9, clipnorm=0.1):
    """Keras SGD(nesterov=True, clipnorm) in float64: v <- m*v - lr*g ; w <- w + m*v - lr*g."""
    w, g, v = (np.asarray(a, np.float64) for a in (w, g, v))
    nrm = math.sqrt(float((g * g).sum()))
    if clipnorm and nrm > clipnorm:
        g = g * (clipnorm / nrm)
    v = momentum * v - lr * g
    return w + momentum * v - lr * g, v


# ----------------------------------------------------------------------------------------------------------------------------------
# seeded synthetic tensors: sizes that hit every path of the slab kernels (slab = 16,384 elements, 16-byte quads + element-wise tail)
# ----------------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 255, 16383, 16384, 16385, 3 * 16384 + 7, 2 * 1024 * 1024 + 5, 40001]
OFFSET_INDEX = 10            # this tensor's w lives 4 bytes off a 16-byte boundary: the unaligned (element-wise) path
NO_DECAY_INDEX = 8           # named ".../bias": excluded from weight decay by the regex below
EXCLUDE = [r"/bias$"]
SMALL_GRAD = {4: 1e-3, 5: 1e-3}      # gradient magnitudes scaled down: these tensors' norms stay below clipnorm = 0.1
CLIPNORM = 0.1


def names():
    return [f"syn/t{i}/{'bias' if i == NO_DECAY_INDEX else 'kernel'}" for i in range(len(SIZES))]


def seeded_weights(seed: int = 20261016):
    rng = np.random.default_rng(seed)
    return [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]


def seeded_gradients(step: int, seed: int = 20261016):
    """Magnitudes log-uniform over four decades (1e-4 .. 1), random signs, about 6 % exact zeros."""
    rng = np.random.default_rng([seed, 1000 + step])
    out = []
    for i, n in enumerate(SIZES):
        g = np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-4.0, 0.0, n) * SMALL_GRAD.get(i, 1.0)
        g[rng.random(n) < 0.06] = 0.0
        out.append(g.astype(np.float32))
    return out


def make_variables(weights):
    """engine.Variable objects on the device holding `weights`; the OFFSET_INDEX one sits one element into its allocation."""
    import torch
    from boosted_detr_amd.engine import Variable, to_device
    out = []
    for i, (name, w) in enumerate(zip(names(), weights)):
        v = Variable(name, (w.size,))
        if i == OFFSET_INDEX:
            buf = torch.zeros(w.size + 4, dtype=torch.float32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            v.value = buf[1: 1 + w.size]
            v.value.copy_(to_device(w))
            assert v.value.data_ptr() % 16 == 4
        else:
            v.value = to_device(w)
        out.append(v)
    return out


def sgd_digests(steps: int = 3):
    """Three steps of the SGD entry point (through training.SGD) on the seeded tensors; SHA-256 of w, velocity and norms per step.
    Used by tests/golden/make_sgd_parent_digests.py (recorded once from the parent build) and by the test that compares."""
    import hashlib
    import torch
    from boosted_detr_amd.training import SGD
    vs = make_variables(seeded_weights())
    opt = SGD(learning_rate=0.05, momentum=0.9, nesterov=True, clipnorm=CLIPNORM)
    opt.build(vs)
    inputs = hashlib.sha256()
    for w in seeded_weights():
        inputs.update(w.tobytes())
    out = {"steps": []}
    for step in range(steps):
        gs = seeded_gradients(step)
        for gv, g in zip(opt.grad_views, gs):
            gv.copy_(torch.from_numpy(g).to(gv.device).view(gv.shape))
            inputs.update(g.tobytes())
        opt.apply_gradients()
        torch.cuda.synchronize()
        dig = lambda ts: hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()
        out["steps"].append({"w": dig([v.value for v in vs]), "v": dig(opt.mom_views), "norms": dig([opt.d_norms])})
    out["inputs"] = inputs.hexdigest()
    return out
