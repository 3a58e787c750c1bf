"""The even-pixel BatchNorm apply of a stage's last unit (bdetr_bn_apply_p16_even_pixels, ops.EVEN_APPLY): the closing BatchNorm +
residual + ReLU pass of conv2_block3 / conv3_block4 / conv4_block6 is read by the next stage's stride-2 1x1 convolutions alone, so it
reads and writes the pixels (2i, 2j) only.

* the kernel against the dense launch: at the even pixels every pair word, fp32 value and mask word is the dense launch's, at every
  other pixel the prefilled buffers are untouched (the pass skips, it does not recompute), and the overflow flag follows the even
  pixels only;
* the entry refuses what its index map cannot serve, and ops.conv_bn takes the dense launch there;
* whole training steps with the path on, off, and on with every unwritten pixel poisoned are bit-identical;
* the compact BatchNorm backward of such a unit does not depend on the mask words of the odd pixels."""
import ctypes

import pytest
import torch

from test_kernels_gpu import dev, rnd
from test_training_gpu import deterministic, small_batch, small_model  # noqa: F401  (deterministic is a fixture)

pytestmark = pytest.mark.gpu

SENTINEL32 = 0x5A5A5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A


def _unit(N, H, W, C, seed):
    """y and the BatchNorm terms of an [N, H, W, C] unit (gamma > 0: a large y gives a large output)."""
    from boosted_detr_amd import kernels as k
    rows = N * H * W
    y = dev(rnd(rows, C, seed=seed) * 2 + 0.3)
    gamma, beta = dev(1 + 0.1 * rnd(C, seed=seed + 1)), dev(0.1 * rnd(C, seed=seed + 2))
    mean, rstd = k.bn_stats(rows, C, k.colstats(y), 1.001e-5, 0.99, True, dev(torch.zeros(C)), dev(torch.ones(C)), like=y)
    return y, (mean, rstd, gamma, beta)


def _residual(form, rows, C, seed):
    """(residual tensor | None, residual_p16, BnAffine | None, tensors to keep alive) of one residual form."""
    from boosted_detr_amd import _lib, kernels as k
    if form == "none":
        return None, 0, None, ()
    if form == "p16":                                   # an identity shortcut: the previous unit's output as its f16 pair
        rf, _ = k.p16_pack(dev(rnd(rows, C, seed=seed).relu_()), want_f16=True, want_bf16=False)
        return rf, 1, None, (rf,)
    ys, p = _unit(1, 1, rows, C, seed)                  # a projection shortcut: its raw convolution output and its BatchNorm
    return ys, 2, _lib.BnAffine(*(t.data_ptr() for t in p)), (ys,) + p


def _launch(even, y, params, res, C, flag, bufs):
    """One direct call of the C entry into caller-owned buffers (o32, of, ob, mask); returns the status."""
    from boosted_detr_amd import _lib, kernels as k
    residual, residual_p16, rbn, _ = res
    L = _lib.lib()
    args = [y.data_ptr(), *(t.data_ptr() for t in params), residual.data_ptr() if residual is not None else None, residual_p16,
            ctypes.byref(rbn) if rbn is not None else None, 1, *(b.data_ptr() for b in bufs), flag.data_ptr(), y.shape[0], C]
    if even is not None:
        return L.bdetr_bn_apply_p16_even_pixels(*args, even[0], even[1], k._stream())
    return L.bdetr_bn_apply_p16(*args, k._stream())


def _buffers(rows, C, fill):
    outs = [torch.full((rows, C), SENTINEL32 if fill else 0, dtype=torch.int32, device="cuda") for _ in range(3)]
    mask = torch.full((rows * C // 256 * 4,), SENTINEL64 if fill else 0, dtype=torch.int64, device="cuda")
    return outs + [mask]


@pytest.mark.parametrize("form", ["p16", "bn", "none"])
@pytest.mark.parametrize("N,H,W,C", [(2, 2, 2, 256), (2, 4, 6, 256), (2, 6, 4, 256), (2, 2, 2, 512), (2, 4, 6, 512), (2, 6, 4, 512), (3, 4, 4, 1024)])
def test_even_pixel_apply_equals_the_dense_launch_and_leaves_odd_pixels_alone(cuda, N, H, W, C, form):
    rows = N * H * W
    y, params = _unit(N, H, W, C, seed=3)
    res = _residual(form, rows, C, seed=11)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    dense, got = _buffers(rows, C, False), _buffers(rows, C, True)
    assert _launch(None, y, params, res, C, flag, dense) == 0
    assert _launch((H, W), y, params, res, C, flag, got) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    even = torch.zeros(N, H, W, dtype=torch.bool, device="cuda")
    even[:, ::2, ::2] = True
    for name, d, g, per_pixel, sentinel in [(n, d, g, C, SENTINEL32) for n, d, g in zip(("out32", "f16 pair", "bf16 pair"), dense, got)] + \
                                           [("mask", dense[3], got[3], C // 256 * 4, SENTINEL64)]:
        d, g = d.view(N, H, W, per_pixel), g.view(N, H, W, per_pixel)
        assert torch.equal(g[even], d[even]), (name, "even pixels differ from the dense launch")
        assert bool((g[~even] == sentinel).all()), (name, "an odd pixel was written")
        assert not bool((d[even] == sentinel).all())            # (the dense values are no sentinel: the comparison above means something)
    # the range guard follows the pixels the pass visits: the same out-of-range value at an odd pixel is never seen
    for (h, w), want in (((0, 1), 0), ((H - 1, W - 1), 0), ((H - 2, W - 2), 1)):
        y2 = y.clone()
        y2.view(N, H, W, C)[N - 1, h, w, C - 3] = 1e30
        flag.zero_()
        assert _launch((H, W), y2, params, res, C, flag, _buffers(rows, C, True)) == 0
        assert int(flag.item()) == want, ((h, w), want)


@pytest.mark.parametrize("N,H,W,C", [(2, 5, 4, 256), (2, 4, 5, 256), (2, 4, 4, 128)])
def test_even_pixel_apply_refuses_odd_maps_and_narrow_channels(cuda, N, H, W, C):
    from boosted_detr_amd import _lib, kernels as k
    y, params = _unit(N, H, W, C, seed=5)
    with pytest.raises(_lib.BdetrError, match="bdetr_bn_apply_p16_even_pixels"):
        k.bn_apply_p16(y, *params, None, True, want_fp32=False, want_f16=True, want_bf16=False, even_pixels=(H, W))
    want = k.bn_apply_p16(y, *params, None, True, want_fp32=False, want_f16=True, want_bf16=False)[1]       # the dense entry serves them
    assert bool(torch.isfinite(k.p16_unpack(want, True)).all())


@pytest.mark.parametrize("H,W,want", [(5, 4, None), (4, 4, (4, 4))])
def test_conv_bn_takes_the_dense_launch_where_the_map_is_odd(cuda, monkeypatch, H, W, want):
    """ops.conv_bn(consumers_read_even_pixels=True) on the training P16 path: the launch that runs, on an odd and on an even map."""
    from boosted_detr_amd import kernels as k, ops
    from boosted_detr_amd.backbone import _ConvBN
    N, Cin, C = 2, 64, 256
    c3 = _ConvBN("t/", "c3", "b3", Cin, C, 1, 1, 0, seed=1)
    launched = []
    real = k.bn_apply_p16

    def spy(*a, **kw):
        launched.append(kw.get("even_pixels"))
        return real(*a, **kw)

    monkeypatch.setattr(k, "bn_apply_p16", spy)
    monkeypatch.setattr(ops, "EVEN_APPLY", True)
    outs = {}
    with k.gemm_precision("split"):
        for flagged in (True, False):
            x = dev(rnd(N, H, W, Cin, seed=1)).relu_()
            ops.attach_packed(x, f16=k.p16_pack(x, want_f16=True, want_bf16=False)[0])
            rf, _ = k.p16_pack(dev(rnd(N, H, W, C, seed=2)).relu_(), want_f16=True, want_bf16=False)
            ops.attach_packed(rf, f16=rf, p16_only=True)
            out = c3([x], training=True, relu=True, residual=rf, want_fp32=False, want_p16=True, next_reads_even_pixels=flagged)
            outs[flagged] = k.p16_unpack(ops.act_info(out).f16, True).view(N, H, W, C)
    torch.cuda.synchronize()
    assert launched == [want, None], launched
    assert torch.equal(outs[True][:, ::2, ::2], outs[False][:, ::2, ::2])


def test_training_steps_are_bit_identical_with_the_even_pixel_apply_on_off_and_poisoned(cuda, deterministic, monkeypatch):  # noqa: F811
    """Three deterministic train_steps from the same weights with ops.EVEN_APPLY on and off: every loss vector and every weight equal.
    A third run keeps the path on and overwrites everything the pass left unwritten - the odd pixels of the f16 pair with NaN patterns,
    their mask words with all-ones - right after each launch: no consumer of a stage-end output may read them into a result (memory
    that merely happens to hold an earlier dense step's values cannot hide one that does)."""
    from boosted_detr_amd import kernels as k, ops
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg, host = small_batch()
    params = O.make_params(cfg, seed=1)
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
             "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    real = k.bn_apply_p16
    engaged = []

    def poisoning(x2d, *a, **kw):
        outs = real(x2d, *a, **kw)
        hw = kw.get("even_pixels")
        if hw is not None:
            H, W = hw
            rows, C = x2d.shape
            odd = torch.ones(rows // (H * W), H, W, dtype=torch.bool, device=x2d.device)
            odd[:, ::2, ::2] = False
            for t, per_pixel in ((outs[1].view(torch.int32), C), (outs[3], C // 256 * 4)):
                t.view(-1, H, W, per_pixel)[odd] = -1
        return outs

    def counting(x2d, *a, **kw):
        if kw.get("even_pixels") is not None:
            engaged.append((tuple(kw["even_pixels"]), x2d.shape[1]))
        return real(x2d, *a, **kw)

    runs = {}
    for name, on, wrapper in (("on", True, counting), ("off", False, counting), ("poisoned", True, poisoning)):
        monkeypatch.setattr(ops, "EVEN_APPLY", on)
        monkeypatch.setattr(k, "bn_apply_p16", wrapper)
        n0 = len(engaged)
        m = small_model()
        m.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
        m.forward_backward(batch)
        m.set_weights_dict(params)
        losses = []
        for _ in range(3):      # name -> the per-image [B] vectors of the step (Model.step_logs), kept on the device
            losses.append({key: [t.detach().clone() for t in v] for key, v in m.train_step(batch).items()})
        torch.cuda.synchronize()
        runs[name] = (losses, {v.name: v.value.detach().clone() for v in m.variables})
        if name == "on":        # the 64 x 64 toy problem: 16 x 16 x 256, 8 x 8 x 512 and 4 x 4 x 1024, once per forward pass
            assert sorted(set(engaged)) == [((4, 4), 1024), ((8, 8), 512), ((16, 16), 256)] and len(engaged) >= 4 * 3, engaged
        if name == "off":
            assert len(engaged) == n0
    assert len(runs["on"][1]) > 100 and all(len(l["loss"]) > 0 for l in runs["on"][0])
    for other in ("off", "poisoned"):
        for step, (a, b) in enumerate(zip(runs["on"][0], runs[other][0])):
            assert a.keys() == b.keys()
            bad = [key for key in a if len(a[key]) != len(b[key]) or not all(torch.equal(s, t) for s, t in zip(a[key], b[key]))]
            assert not bad, (other, step, bad)
        bad = [key for key in runs["on"][1] if not torch.equal(runs["on"][1][key], runs[other][1][key])]
        assert not bad, (other, bad[:5])
    assert all(bool(torch.isfinite(t).all()) for l in runs["on"][0] for t in l["loss"])


def test_compact_batchnorm_backward_ignores_the_mask_words_of_odd_pixels(cuda):
    """bdetr_bn_bwd_p16_even_pixels(dout_compact=1): the gradient is zero at the odd pixels whatever their mask says, and after an
    even-pixel forward those words were never written - the kernel does not read them, and dx does not depend on them."""
    from boosted_detr_amd import kernels as k
    N, H, W, C = 2, 4, 4, 256
    rows = N * H * W
    y, (mean, rstd, gamma, beta) = _unit(N, H, W, C, seed=20)
    bits = k.bn_apply_p16(y, mean, rstd, gamma, beta, dev(rnd(rows, C, seed=23)), True, want_fp32=False, want_f16=True, want_bf16=False, want_mask=True)[3]
    compact = dev(rnd(N * (H // 2) * (W // 2), C, seed=5))
    odd = torch.ones(N, H, W, dtype=torch.bool, device="cuda")
    odd[:, ::2, ::2] = False
    got = []
    for word in (-1, 0):
        b = bits.clone()
        b.view(N, H, W, 4)[odd] = word
        got.append(k.bn_bwd_p16(compact, b, y, mean, rstd, gamma, True, False, beta=beta, want_fp32=True, out_p16=2, even_pixels=(N, H, W), dout_compact=True))
    ref = k.bn_bwd_p16(compact, bits, y, mean, rstd, gamma, True, False, beta=beta, want_fp32=True, out_p16=2, even_pixels=(N, H, W), dout_compact=True)
    for a, b, r in zip(got[0][:4], got[1][:4], ref[:4]):
        assert torch.equal(a, b) and torch.equal(a, r)
    assert float(ref[1].abs().max()) > 0
