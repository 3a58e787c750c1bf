"""Self-tests of the guard arena (tests/_guard.py) on CPU tensors: each of its four conditions can fail.  The "kernels" are
plain-torch stand-ins living in a module of their own, armed exactly as boosted_detr_amd.kernels is on the GPU; a stray access
is spelt with as_strided over the arena's own storage, so nothing here touches memory the test does not own."""
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _guard  # noqa: E402
from _guard import Arena, GuardError  # noqa: E402

standin = types.ModuleType("standin_kernels")
standin.__dict__["__builtins__"] = __builtins__
standin.torch = torch                      # the name the arena swaps for its proxy
standin.real_torch = torch                 # a path the proxy does not cover


def kernel(fn):
    """Re-home fn into the stand-in module: its global `torch` is then the module's, as in kernels.py."""
    g = types.FunctionType(fn.__code__, standin.__dict__, fn.__name__, fn.__defaults__)
    setattr(standin, fn.__name__, g)
    return g


def _at(t, offset):
    """One element at `offset` elements from t's first (negative: in front of it), through t's own storage."""
    return t.as_strided((1,), (1,), t.storage_offset() + offset)


standin._at = _at


@kernel
def doubles(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    return out


@kernel
def writes_past_end(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    _at(out, out.numel()).fill_(1.0)
    return out


@kernel
def writes_before_start(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    _at(out, -1).fill_(1.0)
    return out


@kernel
def folds_margin(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    out.view(-1)[0] += _at(x, -1)[0] * 0          # a load one element in front of the input, times zero
    return out


@kernel
def leaves_last_unwritten(x):
    out = torch.empty_like(x)
    out.view(-1)[:-1] = (x * 2).view(-1)[:-1]
    return out


@kernel
def scribbles_on_input(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    x.view(-1)[3] = 5.0
    return out


@kernel
def outside_arena(x):
    out = real_torch.empty_like(x)                # noqa: F821 - a global of the stand-in module
    out.copy_(x * 2)
    return out


@kernel
def scale_(x):
    x.mul_(2)
    return x


@kernel
def counts(x):
    out = torch.empty(x.numel(), dtype=torch.int32, device=x.device)
    out.copy_(x.view(-1).to(torch.int32))
    return out


@kernel
def counts_short(x):
    out = torch.empty(x.numel(), dtype=torch.int32, device=x.device)
    out[:-1] = x.view(-1)[:-1].to(torch.int32)
    return out


@kernel
def zeroed(x):
    return torch.zeros(x.shape, dtype=torch.float32, device=x.device), torch.zeros_like(x)


def _run(fn, name="x"):
    arena = Arena("cpu")
    host = torch.arange(1, 36, dtype=torch.float32).view(5, 7)
    with arena.armed(standin, dev_modules=()):
        x = arena.place(host, name=name)
        y = getattr(standin, fn.__name__)(x)
    return arena, host, y


def test_correct_standin_passes_and_is_counted():
    arena, host, y = _run(doubles)
    assert arena.verify() == 1 and arena.verify([y]) == 1
    assert torch.equal(y, host * 2)
    assert standin.torch is torch and standin.doubles is doubles          # disarmed again


@pytest.mark.parametrize("fn,cond,side,where", [(writes_past_end, "(a)", "after", "past the end"), (writes_before_start, "(a)", "before", "in front of")])
def test_store_outside_the_output_is_caught(fn, cond, side, where):
    arena, _, y = _run(fn)
    with pytest.raises(GuardError) as e:
        arena.verify([y])
    msg = str(e.value)
    assert cond in msg and "margin %s %s/empty_like" % (side, fn.__name__) in msg and where in msg, msg
    assert "4 byte(s), from 1 to 4 bytes" in msg and "rows of 28 bytes" in msg, msg         # one float next to the interior; a row is 7 floats
    assert "(b)" not in msg and "(c)" not in msg and "(d)" not in msg, msg


def test_load_from_a_margin_that_reaches_the_result_is_caught():
    arena, _, y = _run(folds_margin)
    with pytest.raises(GuardError) as e:
        arena.verify([y])
    msg = str(e.value)
    assert "(d)" in msg and "folds_margin/empty_like" in msg and "1 NaN" in msg and "first at element 0" in msg, msg
    assert "(a)" not in msg, msg


def test_unwritten_element_is_caught():
    arena, _, y = _run(leaves_last_unwritten)
    with pytest.raises(GuardError) as e:
        arena.verify()
    msg = str(e.value)
    assert "(d)" in msg and "leaves_last_unwritten/empty_like" in msg and "first at element 34" in msg, msg
    assert arena.verify(partial=[y]) == 1                                  # a documented partial result is exempt from (d) alone


def test_scribble_on_a_read_only_input_is_caught():
    arena, _, y = _run(scribbles_on_input, name="weights")
    with pytest.raises(GuardError) as e:
        arena.verify([y])
    msg = str(e.value)
    assert "(b)" in msg and "weights" in msg and "first at byte 14" in msg, msg      # element 3 = bytes 12..15; 4.0 -> 5.0 changes byte 14


def test_declared_inplace_operand_may_change():
    arena = Arena("cpu")
    with arena.armed(standin, dev_modules=()):
        x = arena.place(torch.ones(9), name="running sum")
        y = standin.scale_(x)
    arena.verify([y], inplace=[x])
    with pytest.raises(GuardError, match=r"\(b\) read-only input running sum"):
        fresh = Arena("cpu")
        with fresh.armed(standin, dev_modules=()):
            standin.scale_(fresh.place(torch.ones(9), name="running sum"))
        fresh.verify()


def test_result_outside_the_arena_is_caught():
    arena, _, y = _run(outside_arena)
    for returned in (None, [y]):
        with pytest.raises(GuardError) as e:
            arena.verify(returned)
        assert "(c)" in str(e.value) and "outside the arena" in str(e.value), str(e.value)
    assert "outside_arena" in str(arena.results[0][0])


def test_a_case_without_results_fails():
    arena = Arena("cpu")
    with arena.armed(standin, dev_modules=()):
        arena.place(torch.ones(3))
    with pytest.raises(GuardError, match=r"\(c\) no result to guard"):
        arena.verify()


def test_integer_results_two_fills():
    assert _guard.run_guarded("cpu", lambda: standin.counts(torch.arange(10.0)), kernels=standin) == 1
    with pytest.raises(GuardError) as e:
        _guard.run_guarded("cpu", lambda: standin.counts_short(torch.arange(10.0)), kernels=standin)
    assert "(d) integer result of counts_short" in str(e.value) and "first 9, last 9" in str(e.value), str(e.value)


def test_layout_and_fills():
    assert _guard.margin_bytes((3, 4), 4) == 64 << 10                      # floor
    assert _guard.margin_bytes((5, 100), 4) == 256 * 400                   # 256 rows
    assert _guard.margin_bytes((5, 65), 4) % 256 == 0 and _guard.margin_bytes((5, 65), 4) >= 256 * 260
    assert _guard.margin_bytes((98, 8192), 4) == 4 << 20                   # cap
    arena = Arena("cpu")
    with arena.armed(standin, dev_modules=()):
        x = arena.place(torch.ones(3, 5))
        z, zl = standin.zeroed(x)
        e = standin.torch.empty(2, 3, dtype=torch.float32, device="cpu")
    assert x.is_contiguous() and x.data_ptr() % 16 == 0 and z.data_ptr() % 16 == 0
    assert (z == 0).all() and (zl == 0).all() and torch.isnan(e).all()
    assert (arena.place(torch.zeros(4, dtype=torch.int32)) == 0).all()
    other = Arena("cpu", fill=_guard.ALT_FILL)
    with other.armed(standin, dev_modules=()):
        e = standin.torch.empty(3, dtype=torch.int32, device="cpu")
    assert (e == 0x5A5A5A5A).all()
    for b in arena.blocks + other.blocks:
        assert all(bool((region == 0xFF).all()) for _, region in b.sides())
