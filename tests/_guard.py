"""Guard arena: every operand, result and workspace of a kernel call sits inside memory the test owns and has filled
with a known byte, so that a store or a load outside a tensor, or a result element nobody wrote, becomes visible.

    arena = Arena(device)
    with arena.armed():
        x = arena.place(host_tensor)            # or dev(...) of the test modules, rebound to place for the duration
        y = kernels.some_entry_point(x)         # torch.empty / empty_like / zeros inside kernels.py carve from the arena
    arena.verify()                              # or verify([y], inplace=[...])

Layout of one allocation (a flat uint8 tensor):  [ margin 0xFF | interior | margin 0xFF ].  A margin is at least 256 rows
of the operand (the largest row tile; csrc/sgemm.hip reads "up to 255 rows" past the end and relies on the buffer
descriptor to make them zero), at least 64 KiB, a multiple of 256 bytes (the interior keeps the 16-byte alignment
include/bdetr.h requires), and at most 4 MiB.  0xFF bytes read as NaN for f32 and for f16 / bf16 pairs and as -1 for
integers: a load that strays into a margin and reaches the result poisons it.  The interior of a fresh `empty` result
starts as 0xFF too (0x5A in the second run of an integer result), a `zeros` request starts as zeros.

verify() asserts, after a device synchronisation:
  (a) margins    every margin byte of every placed or carved tensor is still 0xFF;
  (b) inputs     the interior of every placed tensor is bit-identical to what was placed, unless it was handed to an
                 in-place parameter (INPLACE_ARGS below, or verify's `inplace`);
  (c) guarded    every result lies inside an arena interior, and there is at least one - a wrapper that allocates
                 through a path the proxy misses fails here instead of passing unguarded;
  (d) written    a floating-point result holds no NaN.  Integer and byte results are compared bit for bit between a run
                 whose fresh interiors start as 0xFF and one whose interiors start as 0x5A (run_guarded): a byte nobody
                 wrote differs.  The integer kernels use no float atomics, so that comparison is exact.

What the method cannot see:
  * a stray store further away than the margin (beyond 256 rows / 64 KiB, or beyond the 4 MiB cap);
  * a stray load whose value is discarded, or is multiplied into nothing that reaches a checked result
    (a NaN times an exact zero IS seen: NaN * 0 = NaN);
  * a packed f16 / bf16 pair result is checked as the f32 words it is carried in: an unwritten word is 0xFFFFFFFF = NaN,
    a written pair whose high half is itself Inf / NaN would also read as NaN;
  * nothing here measures time; no performance claim follows from these tests.

The arena is plain torch and works on CPU tensors as well (tests/test_guard_cpu.py seeds each kind of error there)."""
import contextlib
import functools
import inspect
import sys

import torch

FILL, ALT_FILL = 0xFF, 0x5A                      # 0x5A: SENTINEL32 of test_even_apply_gpu.py
ROW_TILE = 256
MIN_MARGIN, MAX_MARGIN = 64 << 10, 4 << 20
# modules whose `dev` (test_kernels_gpu's, or one with the same signature) is rebound to the arena while it is armed
DEV_MODULES = ("test_kernels_gpu", "test_p16_gpu", "test_precision_gpu", "test_aux_losses_gpu", "_variant_child", "test_panoptic_gpu",
               "test_panoptic_train_gpu", "test_stem_gpu", "test_rowchain_gpu", "test_matcher_gpu", "test_even_apply_gpu",
               "test_memory_bounds_gpu", "test_elementwise_gpu")
ACTIVE = []                                      # the armed arenas, innermost last: a case body reaches its arena as ACTIVE[-1]
# entry point -> parameters the call writes through (caller-supplied destinations, running sums, moving statistics)
INPLACE_ARGS = {
    "axpy_": ("y",), "zero_": ("t",), "relu_mask_apply_": ("x",),
    "conv2d_bwd_data": ("dx",), "conv2d_bwd_weight": ("dw",), "p16_conv2d_bwd_data": ("dx",), "p16_conv2d_bwd_weight": ("dw",),
    "p16_conv2d_bwd_data_masked_accum": ("dx",), "gemm_raw": ("c",), "linear_bwd_data": ("dx",), "linear_bwd_weight": ("dw",),
    "linear_bwd_weight_group": ("dws",), "colsum": ("out",), "colsum_group": ("outs",), "bn_stats": ("moving_mean", "moving_var"),
    "bn_apply": ("out",), "bn_bwd": ("dgamma", "dbeta"), "bn_bwd_p16": ("dgamma", "dbeta"), "bn_rows_apply": ("moving_mean", "moving_var"),
    "bn_rows_bwd": ("dgamma", "dbeta"), "stem_pool_bwd": ("dgamma", "dbeta"), "stem_bwd_weight_s2d": ("dw",),
    "softmax_rows_fwd": ("out",), "softmax_rows_bwd": ("out",), "add_dropout_layernorm_bwd": ("dgamma", "dbeta"),
    "rowchain_reduce": ("dsts",), "add": ("out",), "sum_over_batch": ("out",), "copy_cols": ("dst",),
    "layernorm_act_bwd": ("dgamma", "dbeta"), "conv_weight_unpack": ("dkernel", "dbias"),
}
NOT_RESULTS = ("empty", "overflow_flag")         # an allocator and the process-wide range-guard flag


class GuardError(AssertionError):
    pass


def margin_bytes(shape, itemsize):
    row = (int(shape[-1]) if len(shape) else 1) * itemsize
    m = max(ROW_TILE * row, MIN_MARGIN)
    return min(-(-m // 256) * 256, MAX_MARGIN)


def tensors_in(obj):
    """Every tensor inside nested tuples / lists / dicts."""
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            yield from tensors_in(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from tensors_in(o)


class _Block:
    def __init__(self, name, shape, dtype, device, fill, source=None):
        self.name, self.shape, self.dtype = name, tuple(int(s) for s in shape), dtype
        item = torch.empty((), dtype=dtype).element_size()
        self.row_bytes = max((self.shape[-1] if self.shape else 1) * item, 1)
        n = item
        for s in self.shape:
            n *= s
        self.nbytes, self.margin = n, margin_bytes(self.shape, item)
        self.raw = torch.full((2 * self.margin + n,), FILL, dtype=torch.uint8, device=device)
        body = self.raw[self.margin:self.margin + n]
        if source is not None:
            body.copy_(source.contiguous().view(-1).view(torch.uint8))
            self.snapshot = body.clone()                 # (on the arena's device: comparing there spares a copy of every operand to the host)
        else:
            self.snapshot = None
            if fill != FILL:
                body.fill_(fill)
        self.view = body.view(dtype).view(self.shape)
        self.begin = self.view.data_ptr() if n else self.raw.data_ptr() + self.margin

    def contains(self, t):
        p = t.data_ptr()
        return self.nbytes > 0 and self.begin <= p and p + t.numel() * t.element_size() <= self.begin + self.nbytes

    def sides(self):
        return (("before", self.raw[:self.margin]), ("after", self.raw[self.margin + self.nbytes:]))


class _TorchProxy:
    """Stands in for the name `torch` in one module: empty / empty_like / zeros / zeros_like carve from the arena, all else is torch."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _size(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            return tuple(size[0])
        return tuple(size)

    def _carve(self, what, size, dtype, device, fill):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        f = sys._getframe(2)
        while f.f_code.co_name in ("empty", "<lambda>", "call") and f.f_back is not None:      # kernels.empty, a local shorthand, the recording wrapper
            f = f.f_back
        who = f.f_code.co_name
        return self._arena.carve(size, dtype, torch.device("cpu" if device is None else device), fill, "%s/%s" % (who, what))

    def empty(self, *size, dtype=None, device=None, **kw):
        if kw:
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._carve("empty", self._size(size), dtype, device, self._arena.fill)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if kw:
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._carve("zeros", self._size(size), dtype, device, 0)

    def empty_like(self, t, dtype=None, device=None, **kw):
        if kw:
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._carve("empty_like", tuple(t.shape), t.dtype if dtype is None else dtype, t.device if device is None else device, self._arena.fill)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        if kw:
            return torch.zeros_like(t, dtype=dtype, device=device, **kw)
        return self._carve("zeros_like", tuple(t.shape), t.dtype if dtype is None else dtype, t.device if device is None else device, 0)


class Arena:
    def __init__(self, device="cpu", fill=FILL):
        self.device, self.fill = torch.device(device), fill
        self.blocks, self.results, self._inplace, self._partial = [], [], set(), set()

    # ------------------------------------------------------------------ allocation
    def place(self, t, dtype=None, name=None):
        """Copy a host tensor (or array) into a guarded interior on the arena's device; returns the contiguous interior view."""
        t = torch.as_tensor(t)
        if dtype is not None:
            t = t.to(dtype)
        t = t.detach().contiguous()
        b = _Block(name or "placed#%d %s %s" % (len(self.blocks), tuple(t.shape), str(t.dtype).replace("torch.", "")),
                   t.shape, t.dtype, self.device, FILL, source=t.to(self.device))
        self.blocks.append(b)
        return b.view

    def carve(self, shape, dtype, device, fill, name):
        b = _Block("%s#%d %s %s" % (name, len(self.blocks), tuple(shape), str(dtype).replace("torch.", "")), shape, dtype, device, fill)
        self.blocks.append(b)
        return b.view

    def dev(self, a, dtype=torch.float32):
        """Drop-in for test_kernels_gpu.dev."""
        import numpy as np
        return self.place(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a, dtype)

    # ------------------------------------------------------------------ arming
    def _wrap(self, name, fn):
        sig = inspect.signature(fn)
        writes = INPLACE_ARGS.get(name, ())

        @functools.wraps(fn)
        def call(*args, **kw):
            if writes:
                try:
                    bound = sig.bind(*args, **kw).arguments
                except TypeError:
                    bound = {}
                for p in writes:
                    self.mark_inplace(*tensors_in(bound.get(p)))
            out = fn(*args, **kw)
            if name not in NOT_RESULTS:
                self.results.extend((name, t) for t in tensors_in(out))
            return out
        return call

    def mark_inplace(self, *ts):
        self._inplace.update(t.data_ptr() for t in ts if t is not None)

    def mark_partial(self, *ts):
        """Results that a documented contract leaves partly unwritten; the case checks the written part itself.  Exempt from (d) only."""
        self._partial.update(t.data_ptr() for t in ts if t is not None)

    @contextlib.contextmanager
    def armed(self, kernels=None, dev_modules=DEV_MODULES):
        """While active: the module `kernels` (default boosted_detr_amd.kernels; or a tuple of modules) sees a proxy for `torch` whose
        allocations are carved from this arena, its public functions record what they return and what they write in place, and `dev`
        of the test modules that are already imported resolves to place.  Nothing outside those module namespaces is touched."""
        if kernels is None:
            from boosted_detr_amd import kernels
        modules = tuple(kernels) if isinstance(kernels, (tuple, list)) else (kernels,)
        saved = []

        def swap(mod, attr, value):
            saved.append((mod, attr, getattr(mod, attr)))
            setattr(mod, attr, value)

        try:
            for module in modules:
                swap(module, "torch", _TorchProxy(self))
                for name, fn in list(vars(module).items()):
                    if inspect.isfunction(fn) and fn.__module__ == module.__name__ and not name.startswith("_"):
                        swap(module, name, self._wrap(name, fn))
            for m in dev_modules:
                mod = sys.modules.get(m) or sys.modules.get("tests." + m)
                if mod is not None and hasattr(mod, "dev"):
                    swap(mod, "dev", self.dev)
            ACTIVE.append(self)
            yield self
        finally:
            if ACTIVE and ACTIVE[-1] is self:
                ACTIVE.pop()
            for mod, attr, value in reversed(saved):
                setattr(mod, attr, value)

    # ------------------------------------------------------------------ checks
    def _changed(self, b, side, region, problems):
        bad = (region != FILL).nonzero().view(-1)
        first, last = int(bad[0]), int(bad[-1])
        if side == "before":                     # distance from the interior's first byte, counted backwards
            near, far = region.numel() - last, region.numel() - first
        else:
            near, far = first + 1, last + 1
        problems.append("(a) margin %s %s changed: %d byte(s), from %d to %d bytes (%.2f to %.2f rows of %d bytes) %s the interior"
                        % (side, b.name, bad.numel(), near, far, near / b.row_bytes, far / b.row_bytes, b.row_bytes,
                           "in front of" if side == "before" else "past the end of"))

    def verify(self, returned=None, inplace=(), partial=()):
        """returned: the results (default: every tensor the armed entry points returned).  inplace: placed tensors the calls may
        write.  partial: results that a documented contract leaves partly unwritten (the caller checks those itself): exempt
        from (d) only."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        problems = []
        flags = [(b, side, region) for b in self.blocks for side, region in b.sides()]
        hit = torch.stack([(r != FILL).any() for _, _, r in flags]).cpu() if flags else []
        for (b, side, region), h in zip(flags, hit):
            if bool(h):
                self._changed(b, side, region, problems)
        self.mark_inplace(*inplace)
        for b in self.blocks:
            if b.snapshot is not None and b.nbytes and b.begin not in self._inplace:
                now = b.raw[b.margin:b.margin + b.nbytes]
                if not torch.equal(now, b.snapshot):
                    d = (now != b.snapshot).nonzero().view(-1)
                    problems.append("(b) read-only input %s changed: %d byte(s), first at byte %d" % (b.name, d.numel(), int(d[0])))
        named = [("result", t) for t in tensors_in(returned)] if returned is not None else list(self.results)
        named = [(n, t) for n, t in named if t.device.type == self.device.type and t.numel()]
        if not named:
            problems.append("(c) no result to guard: the case checked nothing")
        skip = {t.data_ptr() for t in tensors_in(partial)} | self._partial
        seen = set()
        for n, t in named:
            key = (t.data_ptr(), t.numel(), t.dtype)
            if key in seen:
                continue
            seen.add(key)
            home = next((b for b in self.blocks if b.contains(t)), None)
            if home is None:
                problems.append("(c) result of %s %s %s lies outside the arena" % (n, tuple(t.shape), t.dtype))
            elif t.is_floating_point() and t.data_ptr() not in skip and bool(torch.isnan(t).any()):
                nan = torch.isnan(t).view(-1).nonzero().view(-1)
                problems.append("(d) result of %s in %s holds %d NaN (unwritten or poisoned), first at element %d, last at %d of %d"
                                % (n, home.name, nan.numel(), int(nan[0]), int(nan[-1]), t.numel()))
        if problems:
            raise GuardError("guard arena: " + "; ".join(problems))
        return len(seen)

    def integer_results(self, partial=()):
        """Host copies, in call order, of the non-floating results (for the two-fill comparison of (d))."""
        skip = {t.data_ptr() for t in tensors_in(partial)} | self._partial
        return [(n, t.detach().cpu().clone()) for n, t in self.results
                if not t.is_floating_point() and t.device.type == self.device.type and t.data_ptr() not in skip]


def run_guarded(device, body, *args, kernels=None, **kw):
    """The whole recipe for a case body that builds its own operands with `dev`: run under a 0xFF arena, verify; if the calls
    returned integer or byte results, run again under a 0x5A arena, verify, and require those results bit-identical."""
    first = Arena(device)
    with first.armed(kernels):
        body(*args, **kw)
    count = first.verify()
    ints = first.integer_results()
    if ints:
        second = Arena(device, fill=ALT_FILL)
        with second.armed(kernels):
            body(*args, **kw)
        second.verify()
        again = second.integer_results()
        assert len(ints) == len(again), (len(ints), len(again))
        for (n, a), (_, b) in zip(ints, again):
            if not torch.equal(a, b):
                d = (a.view(-1) != b.view(-1)).nonzero().view(-1)
                raise GuardError("guard arena: (d) integer result of %s %s differs between the 0xFF and the 0x5A run at %d element(s), first %d, "
                                 "last %d: never written" % (n, tuple(a.shape), d.numel(), int(d[0]), int(d[-1])))
    return count
