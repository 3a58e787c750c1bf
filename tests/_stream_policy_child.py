"""Child process of tests/test_stream_policy_gpu.py: runs every kernel that takes a cache-policy template parameter (csrc/stream.h)
under whatever BDETR_STREAM_POLICY the parent put into the environment - the library reads it once per process - and prints one
JSON line.

    python tests/_stream_policy_child.py kernels | toy

kernels: per case the SHA-256 of every tensor the case produced (a hint changes no value: the parent requires the digests of a
policy-on child to EQUAL those of a policy-off child), and what the guard arena (tests/_guard.py) found - every case, the optimizer's
included, runs between 0xFF margins.  toy: three deterministic training steps of tests/test_training_gpu.small_model; every loss and the SHA-256
of every weight.

The module is also imported by the parent (no GPU work at import time) for the case names."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MARK = "STREAM_POLICY_JSON "
# rows x C of the BatchNorm cases: N = 2, 8 x 8 at both widths, and 130 x 64 = 2080 float4s - 5 workgroups, a grid stride of 1280
# float4s, so the last trip is a partial one (csrc/norm.hip ew_grid(n4, 256, 2))
BN_SHAPES = [(128, 64), (128, 256), (130, 64)]
APPLY_FORMS = ["plain", "res_f16", "res_raw"]
BWD_FORMS = ["out_fp32", "out_bf16", "out_bits", "recompute", "pre_sums"]
CASES = (["apply_p16/%s/%dx%d" % (f, r, c) for r, c in BN_SHAPES for f in APPLY_FORMS] + ["apply_p16/even/128x256"]
         + ["bwd_p16/%s/%dx%d" % (f, r, c) for r, c in BN_SHAPES for f in BWD_FORMS] + ["bwd_p16/compact/128x256"]
         + ["bn_fp32/%dx%d" % s for s in BN_SHAPES] + ["relu_mask_apply/%dx%d" % s for s in BN_SHAPES]
         + ["stem/2x32x32", "weight_pack", "masked_accum/plain", "masked_accum/sums", "masked_accum/compact", "sgd"])


def digest(tensors):
    import torch
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def _bn_operands(rows, C, seed):
    from test_kernels_gpu import dev, rnd
    x = dev(rnd(rows, C, seed=seed) * 2 + 0.3)
    mean, rstd = dev(0.3 + 0.1 * rnd(C, seed=seed + 1)), dev(0.5 + 0.05 * rnd(C, seed=seed + 2).abs())
    gamma, beta = dev(1 + 0.1 * rnd(C, seed=seed + 3)), dev(0.1 * rnd(C, seed=seed + 4))
    return x, mean, rstd, gamma, beta


def apply_case(form, rows, C, arena):
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    x, mean, rstd, gamma, beta = _bn_operands(rows, C, 1)
    short = rnd(rows, C, seed=7)
    if form == "plain":
        return k.bn_apply_p16(x, mean, rstd, gamma, beta, None, True, want_mask=True)
    if form == "res_f16":
        resf = k.p16_pack(dev(short), want_bf16=False)[0]
        return k.bn_apply_p16(x, mean, rstd, gamma, beta, resf, True, residual_p16=True, want_mask=True)
    if form == "res_raw":
        rbn = _bn_operands(rows, C, 11)[1:]
        return k.bn_apply_p16(x, mean, rstd, gamma, beta, dev(short), True, want_mask=True, residual_bn=rbn)
    assert form == "even" and rows == 128
    resf = k.p16_pack(dev(short), want_bf16=False)[0]
    out = k.bn_apply_p16(x, mean, rstd, gamma, beta, resf, True, residual_p16=True, want_mask=True, even_pixels=(8, 8))
    arena.mark_partial(*[t for t in out if t is not None])           # by contract only the even pixels are written
    return out


def bwd_case(form, rows, C, arena):
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    x, mean, rstd, gamma, beta = _bn_operands(rows, C, 21)
    dout = dev(rnd(rows, C, seed=27))
    o32, _, ob, bits = k.bn_apply_p16(x, mean, rstd, gamma, beta, dev(rnd(rows, C, seed=28)), True, want_mask=True)
    kw = dict(beta=beta, want_fp32=True, want_residual_grad=True)
    if form == "out_fp32":
        return k.bn_bwd_p16(dout, o32, x, mean, rstd, gamma, True, False, **kw)
    if form == "out_bf16":
        return k.bn_bwd_p16(dout, ob, x, mean, rstd, gamma, True, False, out_p16=1, **kw)
    if form == "out_bits":
        return k.bn_bwd_p16(dout, bits, x, mean, rstd, gamma, True, False, out_p16=2, **kw)
    if form == "recompute":
        return k.bn_bwd_p16(dout, None, x, mean, rstd, gamma, True, False, **kw)
    if form == "pre_sums":
        pre = (dev(rnd(3, C, seed=29)), dev(rnd(3, C, seed=30)), 3)
        return k.bn_bwd_p16(dout, bits, x, mean, rstd, gamma, True, False, out_p16=2, pre=pre, **kw)
    assert form == "compact" and rows == 128
    compact = dev(rnd(2 * 4 * 4, C, seed=31))
    return k.bn_bwd_p16(compact, bits, x, mean, rstd, gamma, True, False, beta=beta, want_fp32=True, out_p16=2, even_pixels=(2, 8, 8), dout_compact=True)


def fp32_case(rows, C, arena):
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    x, mean, rstd, gamma, beta = _bn_operands(rows, C, 41)
    out = k.bn_apply(x, mean, rstd, gamma, beta, dev(rnd(rows, C, seed=47)), True)
    dout = dev(rnd(rows, C, seed=48))
    return [k.colstats(x)[:2], out, k.bn_bwd(dout, out, x, mean, rstd, gamma, True, False, want_residual_grad=True, beta=beta),
            k.bn_bwd(dout, None, x, mean, rstd, gamma, True, False, beta=beta)[:3]]


def mask_apply_case(rows, C, arena):
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    x, mean, rstd, gamma, beta = _bn_operands(rows, C, 51)
    bits = k.bn_apply_p16(x, mean, rstd, gamma, beta, None, True, want_fp32=False, want_bf16=False, want_mask=True)[3]
    return k.relu_mask_apply_(dev(rnd(rows, C, seed=57)), bits)


def stem_case(arena):
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    y = dev(rnd(2, 32, 32, 64, seed=61) * 2 + 0.3)
    _, mean, rstd, gamma, beta = _bn_operands(8, 64, 62)
    o32, of, tap = k.stem_pool_fwd(y, mean, rstd, gamma, beta, want_fp32=True)
    dpool = dev(rnd(2, 16, 16, 64, seed=63))
    return [o32, of, tap, k.stem_pool_bwd(dpool, tap, y, mean, rstd, gamma, beta), k.stem_pool_bwd(dpool, tap, y, mean, rstd, gamma, beta, dy_p16=True)]


def weight_pack_case(arena):
    import torch
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    shapes = [(64, 1, 1, 256), (64, 3, 3, 64), (256, 1, 1, 64), (8, 7, 7, 8)]
    ws = [dev(rnd(*s, seed=70 + i, scale=0.05)) for i, s in enumerate(shapes)]
    wf = [k.empty(*s, like=w) for s, w in zip(shapes, ws)]
    wt = [k.empty(s[3], s[1], s[2], s[0], like=w) for s, w in zip(shapes, ws)]
    table = torch.tensor([[w.data_ptr(), f.data_ptr(), t.data_ptr(), *s] for w, f, t, s in zip(ws, wf, wt, shapes)], dtype=torch.int64, device="cuda")
    k.p16_pack_conv_weights_multi(table)
    arena.results.extend(("p16_pack_conv_weights_multi", t) for t in wf + wt)
    return wf + wt


def masked_case(form, arena):
    """The masked-accumulate backward-data at I = 512 rows (2 x 16 x 16), J = 256 input channels, R = 64 output channels."""
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    N, H, W, C, K = 2, 16, 16, 256, 64
    g = k.ConvGeom(N, H, W, C, K, 1, 1, 1, 0)
    rows = N * H * W
    _, wt = k.p16_pack_conv_weights(dev(rnd(K, 1, 1, C, seed=81, scale=C ** -0.5)), want_fwd=False)
    _, dyb = k.p16_pack(dev(rnd(N, H, W, K, seed=82)), want_f16=False)
    x, mean, rstd, gamma, beta = _bn_operands(rows, C, 83)
    bits = k.bn_apply_p16(x, mean, rstd, gamma, beta, dev(rnd(rows, C, seed=89)), True, want_fp32=False, want_bf16=False, want_mask=True)[3]
    if form == "plain":
        return k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, dev(rnd(N, H, W, C, seed=90)), bits)
    y2, mean2, rstd2, gamma2, beta2 = _bn_operands(rows, C, 91)
    bits2 = k.bn_apply_p16(y2, mean2, rstd2, gamma2, beta2, dev(rnd(rows, C, seed=97)), True, want_fp32=False, want_bf16=False, want_mask=True)[3]
    ctx = (y2, mean2, rstd2, gamma2, beta2, bits2)
    if form == "sums":
        out = k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, dev(rnd(N, H, W, C, seed=90)), bits, bn_ctx=ctx)
    else:
        assert form == "compact"
        out = k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, k.empty(N, H, W, C, like=dyb), bits, bn_ctx=ctx, old_even=dev(rnd(N, H // 2, W // 2, C, seed=98)))
    dx, (pg, pgx, n) = out
    arena.mark_partial(pg, pgx)                    # rows beyond n are workspace
    return [dx, pg[:n], pgx[:n]]


def sgd_case(arena):
    """Three steps of the fused SGD entry point (sqnorm_kernel, sgd_apply_kernel) through training.SGD on tests/_adamw_ref.py's tensors:
    lengths 1, 3, 5, 255, 16383 ... (no multiple of 4: the element-wise tail next to the float4 path), one tensor 4 bytes off a 16-byte
    boundary.  The weights are placed in the arena; the arena is armed for boosted_detr_amd.training too, so the flat gradient and
    momentum buffers, the slab partials and the norms that SGD.build allocates are carved from it: the non-temporal momentum store,
    the tails and the misaligned tensor all sit between margins."""
    import torch
    import _adamw_ref as R
    from boosted_detr_amd.engine import Variable
    from boosted_detr_amd.training import SGD
    vs, bufs = [], []
    for i, (name, w) in enumerate(zip(R.names(), R.seeded_weights())):
        v = Variable(name, (w.size,))
        if i == R.OFFSET_INDEX:
            buf = arena.place(torch.cat([torch.zeros(1), torch.from_numpy(w), torch.zeros(3)]))
            assert buf.data_ptr() % 16 == 0
            v.value = buf[1: 1 + w.size]
            assert v.value.data_ptr() % 16 == 4
        else:
            buf = arena.place(torch.from_numpy(w))
            v.value = buf
        bufs.append(buf)
        vs.append(v)
    arena.mark_inplace(*bufs)                      # the weights are updated in place
    opt = SGD(learning_rate=0.05, momentum=0.9, nesterov=True, clipnorm=R.CLIPNORM)
    opt.build(vs)
    out = []
    for step in range(3):
        for gv, g in zip(opt.grad_views, R.seeded_gradients(step)):
            gv.copy_(torch.from_numpy(g).to(gv.device).view(gv.shape))
        opt.apply_gradients()
        torch.cuda.synchronize()
        out += [v.value.clone() for v in vs] + [m.clone() for m in opt.mom_views] + [opt.d_norms.clone(), opt.d_partial.clone()]
    # what verify() holds to (c) and (d): everything the entry point read or wrote, all of it inside the arena
    arena.results[:] = [("sgd", t) for t in [v.value for v in vs] + list(opt.mom_views) + [opt.flat_mom, opt.flat_grad, opt.d_norms, opt.d_partial]]
    return out


def run_case(name, arena):
    head, _, rest = name.partition("/")
    if head in ("apply_p16", "bwd_p16"):
        form, _, shape = rest.partition("/")
        rows, C = (int(v) for v in shape.split("x"))
        return (apply_case if head == "apply_p16" else bwd_case)(form, rows, C, arena)
    if head in ("bn_fp32", "relu_mask_apply"):
        rows, C = (int(v) for v in rest.split("x"))
        return (fp32_case if head == "bn_fp32" else mask_apply_case)(rows, C, arena)
    if head == "stem":
        return stem_case(arena)
    if head == "weight_pack":
        return weight_pack_case(arena)
    if head == "sgd":
        return sgd_case(arena)
    assert head == "masked_accum", name
    return masked_case(rest, arena)


def kernels_main():
    import torch
    import _guard
    import test_kernels_gpu  # noqa: F401  (its `dev` is what the arena rebinds)
    from boosted_detr_amd import _lib, kernels, training
    assert torch.cuda.is_available(), "the stream-policy child needs a GPU"
    out = {"policy": int(_lib.lib().bdetr_stream_policy()), "cases": {}}
    for name in CASES:
        arena = _guard.Arena("cuda")
        with arena.armed((kernels, training) if name == "sgd" else None):
            res = run_case(name, arena)
        guard = None
        try:
            arena.verify()
        except _guard.GuardError as e:
            guard = str(e)[:1500]
        out["cases"][name] = {"digest": digest(list(_guard.tensors_in(res))), "guard": guard}
        del arena, res
    print(MARK + json.dumps(out), flush=True)


def toy_main():
    import torch
    from boosted_detr_amd import _lib
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    from test_training_gpu import small_batch, small_model
    assert torch.cuda.is_available(), "the stream-policy child needs a GPU"
    K.set_deterministic(True)
    from boosted_detr_amd.engine import to_device
    cfg, host = small_batch()
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
             "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    m = small_model()
    m.compile(optimizer=SGD(1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    m.forward_backward(batch)                      # build
    m.set_weights_dict(O.make_params(cfg, seed=1))
    losses = [float(m.logs_to_host(m.train_step(batch))["loss"]) for _ in range(3)]
    torch.cuda.synchronize()
    weights = {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in m.get_weights_dict().items()}
    print(MARK + json.dumps({"policy": int(_lib.lib().bdetr_stream_policy()), "losses": [x.hex() for x in losses], "weights": weights}), flush=True)


if __name__ == "__main__":
    {"kernels": kernels_main, "toy": toy_main}[sys.argv[1]]()
