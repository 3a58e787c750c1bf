"""Direct parity of the kernels.py entry points that only whole-model tests reached (csrc/elementwise.hip): add, axpy_, tanh_bwd,
relu_bwd, add_bcast_rows, sum_over_batch, zero_, tokens_prepare, flag_nonfinite.  Every case runs inside the guard arena
(tests/_guard.py): operands and results sit between 0xFF margins, fresh results start as NaN.

Lengths 1, 3, 255, 257, 1025 sit below, at and above one 256-thread block.  An operation that is one fp32 rounding (or none) is
compared bit for bit with the same fp32 formula in torch; everything else with `close` at 2e-5 x max|fp64 reference|."""
import numpy as np
import pytest
import torch

from _guard import Arena
from test_kernels_gpu import close, rnd

pytestmark = pytest.mark.gpu
LENGTHS = [1, 3, 255, 257, 1025]


@pytest.fixture
def arena(cuda):
    a = Arena(cuda)
    with a.armed():
        yield a


@pytest.mark.parametrize("n", LENGTHS)
def test_add_tanh_bwd_relu_bwd(arena, n):
    from boosted_detr_amd import kernels as k
    a, b = rnd(n, seed=1), rnd(n, seed=2)
    got = k.add(arena.place(a), arena.place(b))
    assert torch.equal(got.cpu(), a + b)                                    # one rounding
    close(got, a.double() + b.double())
    out = arena.place(torch.full((n,), float("nan")))
    assert k.add(arena.place(a), arena.place(b), out=out) is out and torch.equal(out.cpu(), a + b)
    y = torch.tanh(rnd(n, seed=3) * 2)
    y[0] = 1.0                                                              # a saturated unit: gradient exactly 0
    dx = k.tanh_bwd(arena.place(y), arena.place(b))
    close(dx, b.double() * (1 - y.double() ** 2))
    assert float(dx[0]) == 0.0
    yr = rnd(n, seed=4).relu()
    yr[0] = 0.0                                                             # y = 0 gives 0 ...
    if n > 2:
        yr[1] = -0.0                                                        # ... and so does -0.0
    want = torch.where(yr > 0, b, torch.zeros(()))
    dr = k.relu_bwd(arena.place(yr), arena.place(b))
    assert torch.equal(dr.cpu(), want) and float(dr[0]) == 0.0              # a selection: exact
    if n > 2:
        assert float(dr[1]) == 0.0
    assert arena.verify([got, out, dx, dr], inplace=[out]) == 4


@pytest.mark.parametrize("alpha", [0.0, -0.5, 3.0])
@pytest.mark.parametrize("n", LENGTHS)
def test_axpy(arena, n, alpha):
    from boosted_detr_amd import kernels as k
    x, y0 = rnd(n, seed=1), rnd(n, seed=2)
    y = arena.place(y0)
    assert k.axpy_(alpha, arena.place(x), y) is y
    close(y, y0.double() + alpha * x.double())
    if alpha == 0.0:
        assert torch.equal(y.cpu(), y0)                                     # y + 0 * x: exact for finite x
    elif alpha == -0.5:
        assert torch.equal(y.cpu(), y0 + alpha * x)                         # a power of two: the product is exact, one rounding either way
    assert arena.verify([y], inplace=[y]) == 1


@pytest.mark.parametrize("rows,rowlen", [(1, 1), (7, 3), (33, 257)])
def test_add_bcast_rows(arena, rows, rowlen):
    from boosted_detr_amd import kernels as k
    a, row = rnd(rows, rowlen, seed=1), rnd(rowlen, seed=2)
    out = k.add_bcast_rows(arena.place(a), arena.place(row))
    assert torch.equal(out.cpu(), a + row)
    close(out, a.double() + row.double())
    assert arena.verify([out]) == 1


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", LENGTHS)
def test_sum_over_batch(arena, n, batch, accumulate):
    """Both values of the C entry's `accumulate` (kernels.sum_over_batch passes 0; the 1 goes through the C ABI)."""
    from boosted_detr_amd import _lib, kernels as k
    x, base = rnd(batch, n, seed=1), rnd(n, seed=2)
    ref = x.double().sum(0)
    if accumulate:
        out = arena.place(base)
        _lib.check(_lib.lib().bdetr_sum_over_batch(arena.place(x).data_ptr(), out.data_ptr(), batch, n, 1, k._stream()), "sum_over_batch")
        ref = ref + base.double()
    else:
        out = arena.place(torch.full((n,), float("nan")))                   # the destination's old content must not matter
        assert k.sum_over_batch(arena.place(x), n, out=out) is out
        fresh = k.sum_over_batch(arena.place(x), n)
        assert torch.equal(fresh, out)
    close(out, ref)
    assert arena.verify([out] if accumulate else [out, fresh], inplace=[out]) == 2 - accumulate


# bdetr_zero_bytes (csrc/elementwise.hip): head = bytes up to the next 16-byte boundary, body = 16-byte stores, tail = bytes.
#   offset 1..3, length <= 4 - offset            -> head only (the "tiny and unaligned" launch)
#   offset 0, length 4 or 8                      -> body only
#   offset 0, length 1..3                        -> tail only; length 5..7, 9, 1027 -> body + tail
#   offset 1..3, length > 4 - offset             -> head, then body and / or tail: e.g. (1, 9) = 3 + 4 + 2 floats, (3, 1027) = 1 + 1024 + 2
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_zero_respects_its_boundaries(arena, offset):
    from boosted_detr_amd import kernels as k
    lengths = list(range(1, 10)) + [1027]
    paths = set()
    held = []
    for n in lengths:
        buf = arena.place(torch.full((4 + offset + n + 8,), 7.0))          # placed 16-byte aligned; the target starts 4 + offset floats in
        assert buf.data_ptr() % 16 == 0
        t = buf[4 + offset:4 + offset + n]
        assert t.data_ptr() % 16 == 4 * offset
        assert k.zero_(t) is t
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[4 + offset:4 + offset + n] == 0).all()), (offset, n)
        assert bool((host[:4 + offset] == 7.0).all()) and bool((host[4 + offset + n:] == 7.0).all()), (offset, n, "a neighbour was touched")
        head = (4 - offset) % 4
        paths.add("head only" if head >= n else ("head+" if head else "") + ("body" if (n - head) // 4 else "") + ("+tail" if (n - head) % 4 else ""))
        held.append(buf)
    if offset == 0:
        assert {"body", "+tail", "body+tail"} <= paths, paths
    else:
        assert {"head only", "head+body+tail"} <= paths, paths
    assert arena.verify([b[4 + offset:] for b in held], inplace=held) == len(held)


def test_tokens_prepare(arena):
    from boosted_detr_amd import kernels as k
    C, A = 10, 6
    big = 2 ** 31 - 1
    cat = torch.tensor([[0, 1, C - 1, C], [-1, big, 5, 0]], dtype=torch.int32)           # PAD, OOV, last, first one outside, negative, INT_MAX
    att = torch.tensor([[[0, 0, 0], [1, 2, 2], [A - 1, A - 1, A - 1], [A, 3, 0]],         # duplicate slots; A is outside -> 1
                        [[-1, big, 4], [5, 4, 3], [2, 0, 2], [0, 1, 0]]], dtype=torch.int32)
    got_cat, hot = k.tokens_prepare(arena.place(cat), arena.place(att), C, A)
    want_cat = torch.where((cat >= 0) & (cat < C), cat, torch.ones((), dtype=torch.int32))
    assert got_cat.dtype == torch.int32 and torch.equal(got_cat.cpu(), want_cat)
    ids = torch.where((att >= 0) & (att < A), att, torch.ones((), dtype=torch.int32)).long()
    want_hot = torch.nn.functional.one_hot(ids, A).amax(2).float()
    assert torch.equal(hot.cpu(), want_hot)
    assert want_hot[0, 0].tolist() == [1, 0, 0, 0, 0, 0] and want_hot[0, 3].tolist() == [1, 1, 0, 1, 0, 0]
    # one slot given as [B, M]; a [B, M, 1] category tensor
    c3, h1 = k.tokens_prepare(arena.place(cat.view(2, 4, 1)), arena.place(att[..., 0].contiguous()), C, A)
    assert torch.equal(c3.cpu(), want_cat)
    assert torch.equal(h1.cpu(), torch.nn.functional.one_hot(ids[..., 0], A).float())
    # no slots at all: the multi-hot matrix is all zero (the attribute operand is then empty, its pointer null)
    c0, h0 = k.tokens_prepare(arena.place(cat), arena.place(torch.zeros(2, 4, 0, dtype=torch.int32)), C, A)
    assert torch.equal(c0.cpu(), want_cat) and tuple(h0.shape) == (2, 4, A) and float(h0.abs().max()) == 0.0
    # the integer result under the second fill: a byte nobody wrote would differ
    second = Arena(arena.device, fill=0x5A)
    with second.armed():
        again, hot2 = k.tokens_prepare(second.place(cat), second.place(att), C, A)
    second.verify([again, hot2])
    assert torch.equal(again, got_cat) and torch.equal(hot2, hot)
    assert arena.verify([got_cat, hot, c3, h1, c0, h0]) == 6


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_flag_nonfinite_raises_for_every_position(arena, bad, where):
    from boosted_detr_amd import kernels as k
    n = 1025
    x = rnd(n, seed=1)
    x[{"first": 0, "middle": 513, "last": n - 1}[where]] = bad
    k.overflow_flag().zero_()
    xd = arena.place(x)
    k.flag_nonfinite(xd)
    assert k.read_and_clear_overflow()
    assert arena.verify([xd], partial=[xd]) == 1                            # (the operand itself: margins and bit-identity; it holds the NaN on purpose)


@pytest.mark.parametrize("n", LENGTHS)
def test_flag_nonfinite_stays_down_for_finite_data(arena, n):
    """The kernel's threshold is |x| <= 3.0e38, not FLT_MAX (3.4028e38): pinned as it is.  Values in (3.0e38, FLT_MAX] are finite and
    raise the flag all the same; nothing in a training step comes near either bound."""
    from boosted_detr_amd import kernels as k
    x = rnd(n, seed=1)
    x[0] = 3.0e38
    x[n - 1] = -3.0e38 if n > 1 else 3.0e38
    k.overflow_flag().zero_()
    xd = arena.place(x)
    k.flag_nonfinite(xd)
    assert not k.read_and_clear_overflow()
    above = x.clone()
    above[n // 2] = float(np.nextafter(np.float32(3.0e38), np.float32(np.inf)))
    k.flag_nonfinite(arena.place(above))
    assert k.read_and_clear_overflow()
    assert arena.verify([xd]) == 1
