"""The fp64 residual-unit reference of tests/_resunit_ref.py checked on the host: it equals the obvious torch composite, injected
decisions are a no-op where they are its own, its fp32 run (the tolerance yardstick of tests/test_resunit_gpu.py) takes the same ReLU
decisions as the fp64 run, and the bit-mask decoder inverts the encoder."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resunit_ref as R


def _inputs(geometry, seed=1):
    H, W = R.POOL_HW[geometry]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, H, W, 64, generator=g).relu()                     # a pooled ReLU output: non-negative
    cout = 4 * R.STAGES[-1][0]
    oh, ow = H, W
    for _, _, stride in R.unit_strides(R.STAGES):
        oh, ow = (oh - 1) // stride + 1, (ow - 1) // stride + 1
    gout = torch.randn(2, oh, ow, cout, generator=g)
    return x.numpy(), gout.numpy()


def _composite(x, blocks):
    """The same network from F.conv2d / F.batch_norm / torch.relu, in NCHW."""
    def cb(t, p, stride, pad):
        y = F.conv2d(t, p["kernel"].permute(0, 3, 1, 2), p["bias"], stride=stride, padding=pad)
        return F.batch_norm(y, None, None, p["gamma"], p["beta"], training=True, eps=R.EPS)

    t = x.permute(0, 3, 1, 2)
    for blk, (_, _, stride) in zip(blocks, R.unit_strides(R.STAGES)):
        sc = cb(t, blk["short"], stride, 0) if blk["short"] is not None else t
        y = torch.relu(cb(t, blk["c1"], stride, 0))
        y = torch.relu(cb(y, blk["c2"], 1, 1))
        t = torch.relu(cb(y, blk["c3"], 1, 0) + sc)
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("geometry", ["even", "odd"])
def test_reference_equals_the_torch_composite(geometry):
    blocks = R.random_blocks(R.STAGES, seed=3)
    x, gout = _inputs(geometry)
    rec, grads = R.run(R.STAGES, x, blocks, gout=gout)
    p = R.leaves(blocks)
    out = _composite(torch.as_tensor(x).double(), p)
    last = R.unit_name(len(blocks) - 1) + ".c3"
    assert out.shape == rec[last].shape == torch.Size(gout.shape)
    assert R.deviation(out.detach(), rec[last]) < 1e-12
    out.backward(torch.as_tensor(gout).double())
    top = max(float(g.abs().max()) for g in grads.values())
    for i, blk in enumerate(p):
        for layer in R.LAYERS:
            for n, t in (blk[layer] or {}).items():
                assert R.deviation(t.grad, grads[f"u{i}.{layer}.{n}"], floor=1e-2 * top) < 1e-10, (i, layer, n)
    # a convolution bias under train-mode BatchNorm has no gradient but round-off: why gradient scales get a floor
    assert max(float(grads[k].abs().max()) for k in grads if k.endswith(".bias")) < 1e-9 * top


def test_injecting_its_own_decisions_changes_nothing():
    blocks = R.random_blocks(R.STAGES, seed=3)
    x, gout = _inputs("even")
    rec, grads = R.run(R.STAGES, x, blocks, gout=gout)
    own = {k[:-4]: rec[k] > 0 for k in rec if k.endswith(".pre")}
    assert len(own) == 3 * len(blocks)
    rec2, grads2 = R.run(R.STAGES, x, blocks, decisions=own, gout=gout)
    assert all(torch.equal(rec[k], rec2[k]) for k in rec) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    # ... and other decisions do change it: the argument is not ignored
    flipped = dict(own)
    flipped["u2.c3"] = ~own["u2.c3"]
    rec3, _ = R.run(R.STAGES, x, blocks, decisions=flipped)
    assert not torch.equal(rec3["u3.c1"], rec["u3.c1"])


@pytest.mark.parametrize("geometry", ["even", "odd"])
def test_fp32_run_takes_the_fp64_decisions(geometry):
    """The cap of the stage-parity test: a device decision may differ from the fp64 one on at most 1e-4 of all ReLU inputs.  The fp32
    run of the reference itself stays far below it, so the cap binds a broken forward pass only; and its output error e32 is what
    the allowances are multiples of."""
    blocks = R.random_blocks(R.STAGES, seed=3)
    x, _ = _inputs(geometry)
    r64, _ = R.run(R.STAGES, x, blocks)
    r32, _ = R.run(R.STAGES, x, blocks, dtype=torch.float32)
    pres = [k for k in r64 if k.endswith(".pre")]
    total = sum(r64[k].numel() for k in pres)
    differ = sum(int(((r64[k] > 0) != (r32[k] > 0)).sum()) for k in pres)
    assert total > 1e5 and differ <= 1e-4 * total, (differ, total)
    e32 = max(R.deviation(r32[k], r64[k]) for k in r64 if not k.endswith(".pre"))
    assert 0 < e32 < 1e-4, e32


@pytest.mark.parametrize("numel", [4, 256, 260, 408, 51 * 8, 130 * 64])
def test_mask_words_round_trip(numel):
    g = torch.Generator().manual_seed(numel)
    keep = torch.rand(numel, generator=g) > 0.5
    words = R.mask_encode(keep)
    assert words.dtype == torch.int64 and words.numel() == ((numel // 4 + 63) // 64) * 4
    assert torch.equal(R.mask_decode(words, numel), keep)


def test_mask_word_layout():
    """Element e of float4 index i lives in word (i >> 6) * 4 + e, bit i & 63 (csrc/norm.hip)."""
    numel = 4 * 130
    for i, e in ((0, 0), (0, 3), (63, 1), (64, 0), (129, 2)):
        words = np.zeros(((130 + 63) // 64) * 4, dtype=np.uint64)
        words[(i >> 6) * 4 + e] = np.uint64(1) << np.uint64(i & 63)
        got = R.mask_decode(torch.from_numpy(words.view(np.int64)), numel)
        want = torch.zeros(numel, dtype=torch.bool)
        want[4 * i + e] = True
        assert torch.equal(got, want), (i, e)
        assert torch.equal(R.mask_encode(want), torch.from_numpy(words.view(np.int64)))
