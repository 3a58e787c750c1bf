"""CPU tests of the host logic that needs no kernels: tokenizers, schedules, variable layout
conversion, tape accumulation order, bench helpers, and the 2-rank gloo gradient all-reduce."""
import os
import subprocess
import sys

import numpy as np
import pytest

def _free_port() -> str:
    """A port nobody listens on right now (fixed numbers collided with other jobs sharing the box's network namespace: one abort in
    RCCL's bootstrap in round 4)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tokenization_string_lookup_semantics(monkeypatch):
    from boosted_detr_amd import engine, tokenizers
    import torch
    monkeypatch.setattr(engine, "to_device", lambda a, dtype=torch.float32: torch.as_tensor(np.asarray(a)).to(dtype))
    monkeypatch.setattr(tokenizers, "to_device", engine.to_device)
    vocab = {"category": ["cat", "dog"], "attribute": ["red", "big", "old"]}
    tok = tokenizers.Tokenization(vocab)
    assert tok.vocab_size_dict() == {"category": 4, "attributes": 5}
    cat = np.array([[["dog"], ["<PAD>"], ["zebra"]]], dtype=object)
    att = np.array([[["big", "red"], ["<PAD>", "<PAD>"], ["old", "<PAD>"]]], dtype=object)
    ids, hot = tok([cat, att])
    assert ids.tolist() == [[3, 0, 1]]                       # vocab from 2, PAD=0, OOV=1
    assert hot[0, 0].tolist() == [0, 0, 1, 1, 0]
    assert hot[0, 1].tolist() == [1, 0, 0, 0, 0]             # PAD slots set bit 0 (tokenizers.py:76)
    assert hot[0, 2].tolist() == [1, 0, 0, 0, 1]
    ids2, _ = tok([np.array([[3, 0, 1]], np.int32), np.zeros((1, 3, 2), np.int32)])
    assert ids2.tolist() == [[3, 0, 1]]                      # pre-tokenised ids pass through


def test_inverse_tokenization_strings():
    import torch
    from boosted_detr_amd import tokenizers
    vocab = {"category": ["cat", "dog"], "attribute": ["red", "big", "old"]}
    inv = tokenizers.InverseTokenization(vocab)
    cat = torch.tensor([[[0.1, 0.1, 0.2, 0.6], [0.7, 0.1, 0.1, 0.1], [0.25, 0.25, 0.25, 0.25]]])
    att = torch.tensor([[[0.1, 0.2, 0.9, 0.6, 0.1], [0.0, 0.0, 0.0, 0.0, 0.0], [0.9, 0.9, 0.1, 0.1, 0.5]]])
    c, a = inv([cat, att])
    assert c[0, :, 0].tolist() == ["dog", "<PAD>", "<PAD>"]  # argmax takes the first maximum on ties
    # the reference's regex clean-up (tokenizers.py:146-155) leaves a trailing comma when PAD slots follow: kept
    assert a[0, 0, 0] == "red, big," and a[0, 1, 0] == "" and a[0, 2, 0] == "old"


def test_cosine_decay_restarts_matches_oracle():
    from boosted_detr_amd.training import CosineDecayRestarts
    from oracle import detr_oracle as O
    s = CosineDecayRestarts(1e-3, 4000, m_mul=0.95, alpha=0.1)
    for step in (0, 1, 1999, 4000, 4001, 11999, 12000, 30000):
        assert abs(s(step) - O.cosine_decay_restarts(step, 1e-3, 4000, 2.0, 0.95, 0.1)) < 1e-15


def test_variable_layout_roundtrip(monkeypatch):
    import torch
    from boosted_detr_amd import engine
    monkeypatch.setattr(engine, "to_device", lambda a, dtype=torch.float32: torch.as_tensor(np.asarray(a)).to(dtype).contiguous())
    rng = np.random.default_rng(0)
    v = engine.Variable("c/kernel", (7, 7, 3, 64), kind="conv_kernel", pad_in_channels=1)
    k = rng.standard_normal((7, 7, 3, 64)).astype(np.float32)
    v.assign(k)
    assert tuple(v.value.shape) == (64, 7, 7, 4) and float(v.value[..., 3].abs().max()) == 0.0
    assert np.array_equal(v.numpy(), k)
    d = engine.Variable("d/kernel", (5, 9), kind="dense_kernel")
    w = rng.standard_normal((5, 9)).astype(np.float32)
    d.assign(w)
    assert tuple(d.value.shape) == (9, 5) and np.array_equal(d.numpy(), w)


def test_gradient_tag_rules_of_a_dense_contribution():
    """engine.GradInfo: a dense contribution added to an accumulated gradient ends its BatchNorm partial sums (both kinds) and its
    even-pixel tag - except that a further stride-2 1x1 contribution on the same (N, H, W) keeps the tag - and leaves ownership and a
    lazy mask alone; reading the record of an untagged tensor allocates nothing on it."""
    import torch
    from boosted_detr_amd.engine import GradInfo, dense_contribution, info, own, tag
    plain = torch.zeros(2, 4, 4, 8)
    empty = info(plain)
    assert empty is info(None) and empty is info(torch.zeros(1)) and "_grad_info" not in plain.__dict__
    assert (empty.owned, empty.lazy_mask, empty.compact_even, empty.even_pixels, empty.bnb_parts, empty.bnb_parts_shortcut) == (False,) + (None,) * 5
    dense_contribution(plain)                       # nothing to drop, and the shared empty record stays empty and unattached
    assert "_grad_info" not in plain.__dict__ and info(plain) is empty and empty.even_pixels is None and empty.bnb_parts is None

    def tagged():
        g = own(torch.zeros(2, 4, 4, 8))
        r = tag(g)
        assert isinstance(r, GradInfo) and r is info(g) and r is tag(g) and r is not empty
        r.lazy_mask, r.even_pixels, r.bnb_parts, r.bnb_parts_shortcut = torch.ones(4, dtype=torch.int64), (2, 4, 4), ("g", "gx", 3), ("s",)
        return g, r

    g, r = tagged()
    mask = r.lazy_mask
    dense_contribution(g)
    assert r.bnb_parts is None and r.bnb_parts_shortcut is None and r.even_pixels is None
    assert r.owned is True and r.lazy_mask is mask and info(g) is r
    g, r = tagged()
    mask = r.lazy_mask
    dense_contribution(g, keep_even=(2, 4, 4))      # a stride-2 1x1 contribution on the same map writes the even pixels only
    assert r.even_pixels == (2, 4, 4) and r.bnb_parts is None and r.bnb_parts_shortcut is None and r.owned is True and r.lazy_mask is mask
    g, r = tagged()
    dense_contribution(g, keep_even=(2, 8, 8))      # ... on another map it is a dense contribution like any other
    assert r.even_pixels is None and r.bnb_parts is None and r.bnb_parts_shortcut is None
    with pytest.raises(AttributeError):
        r.lazy_msak = None                          # a misspelt field is an error, not a silently ignored tag


def test_initializers_statistics():
    from boosted_detr_amd.engine import initializer
    w = initializer("glorot_normal")("x", (256, 256))
    assert abs(w.std() - np.sqrt(2.0 / 512)) < 2e-3 and np.abs(w).max() <= 2.0 * np.sqrt(2.0 / 512) / 0.8796 + 1e-6
    w = initializer("he_normal")("y", (256, 1024))
    assert abs(w.std() - np.sqrt(2.0 / 256)) < 2e-3
    assert initializer("zeros")("z", (4,)).sum() == 0 and initializer("ones")("o", (4,)).sum() == 4


def test_positional_init_matches_oracle():
    from boosted_detr_amd.transformers import positional_init
    from oracle import detr_oracle as O
    assert np.array_equal(positional_init(3, 4, 16), O.positional_init(3, 4, 16))


def test_bench_batch_generator_matches_oracle_generator():
    sys.path.insert(0, ROOT)
    import bench
    from oracle import detr_oracle as O
    a = bench.make_batch(3, 16, 16, 100, 82, seed=1234)
    b = O.make_batch(O.Config(image_size=(16, 16), num_categories=82, num_attributes=3), 3, 100, seed=1234)
    for k in ("image", "category", "bbox", "num_objects"):
        assert np.array_equal(a[k], b[k]), k
    assert 1 <= bench.usable_cores() <= 16


def test_bench_dump_outputs_float32_bounded_and_seeded(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the step's per-image vectors (one file per weak learner), extra outputs (the panoptic masks) and a
    variable sample drawn at the same positions every run, float32, within 64 MB."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    assert bench.DUMP_SAMPLE * 4 <= (64 << 20) - (1 << 20)     # the shipped sample leaves room for the per-image vectors
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    g = torch.Generator().manual_seed(0)
    logs = {"loss": [torch.rand(4, dtype=torch.float64, generator=g)], "IOU": [torch.rand(4, generator=g), torch.rand(4, generator=g)]}
    model = type("M", (), {"variables": [type("V", (), {"value": torch.randn(s, generator=g)})() for s in (700, 600, 3)],
                           "step_logs": lambda self: logs})()
    extra = {"panoptic_masks": torch.randn(2, 3, 5, generator=g)}
    names = bench.dump_outputs(model, str(tmp_path / "a"), extra)
    assert names == ["IOU_0", "IOU_1", "loss", "panoptic_masks", "variables_sample"]
    bench.dump_outputs(model, str(tmp_path / "b"), extra)
    flat = torch.cat([v.value for v in model.variables]).numpy()
    for n in names:
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "a" / "IOU_1.npy"), logs["IOU"][1].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "panoptic_masks.npy"), extra["panoptic_masks"].numpy())
    s = np.load(tmp_path / "a" / "variables_sample.npy")
    assert s.shape == (1000,) and np.isin(s, flat).all() and len(np.unique(s)) == 1000


_DP_SCRIPT = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from boosted_detr_amd.training import DataParallel
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
dp = DataParallel()
dp.BUCKET_ELEMS = 1000                      # several buckets
rng = np.random.default_rng(dp.rank)
flat = torch.from_numpy(rng.standard_normal(4321).astype(np.float32))
want = sum(np.random.default_rng(r).standard_normal(4321).astype(np.float32) for r in range(dp.world))
dp.allreduce_(flat)
assert np.allclose(flat.numpy(), want, atol=1e-6), "allreduce mismatch"
class V:  # broadcast path
    pass
v = V(); v.value = torch.full((5,), float(dp.rank))
dp.broadcast_variables([v])
assert float(v.value.sum()) == 0.0
# bucketed all-reduce launched from the backward pass (grad_ready) - buckets count from the END of the flat buffer
class Opt: pass
sizes = [1200, 800, 1500, 700, 796]
offs = np.concatenate([[0], np.cumsum(sizes)])
flat = torch.zeros(int(offs[-1]))
vs = []
for i, sz in enumerate(sizes):
    q = V(); q.name = "v%d" % i; q.grad_buf = flat[int(offs[i]): int(offs[i]) + sz]; q.grad = None; q._grad_flat = flat
    vs.append(q)
opt = Opt(); opt.flat_grad = flat; opt.vars = vs
dp2 = DataParallel(); dp2.BUCKET_ELEMS = 1000
for step in range(4):
    flat.zero_()
    dp2.begin_step(opt, None, None)
    early = 0
    for i in reversed(range(len(vs))):                      # backward order: last variable first
        q = vs[i]
        q.grad_buf.copy_(torch.full((sizes[i],), float((dp2.rank + 1) * (i + 1) + step)))
        q.grad = q.grad_buf
        dp2.grad_ready(q)
        if i == 2:                                          # a shared variable: second contribution lands later
            q.grad_buf.add_(0.5)
            dp2.grad_ready(q)
        early = max(early, sum(dp2._launched)) if dp2._expected is not None and dp2._active else early
    dp2.finish(flat)
    for i, sz in enumerate(sizes):
        want = sum((r + 1) * (i + 1) + step + (0.5 if i == 2 else 0.0) for r in range(dp2.world))
        got = flat[int(offs[i]): int(offs[i]) + sz]
        assert torch.all(got == want), (step, i, float(got[0]), want)
    assert (early > 0) == (step >= 1), (step, early)        # step 0 calibrates the contribution counts, later steps overlap
# The trainable set changed (freeze / unfreeze): Model.forward_backward rebuilds the optimizer BEFORE begin_step, so the step is
# armed on the new buffer, runs one calibration step without early launches, then overlaps again - every sum right throughout.
keep = [0, 2, 4]
sizes2 = [sizes[i] for i in keep]
offs2 = np.concatenate([[0], np.cumsum(sizes2)])
flat2 = torch.zeros(int(offs2[-1]))
vs2 = []
for j, i in enumerate(keep):
    q = vs[i]; q.grad_buf = flat2[int(offs2[j]): int(offs2[j]) + sizes2[j]]; q.grad = None; q._grad_flat = flat2
    vs2.append(q)
opt.flat_grad = flat2; opt.vars = vs2
for step in range(3):
    flat2.zero_()
    dp2.begin_step(opt, None, None)
    early = 0
    for j in reversed(range(len(vs2))):
        q = vs2[j]
        q.grad_buf.copy_(torch.full((sizes2[j],), float((dp2.rank + 1) * (j + 1) + step)))
        q.grad = q.grad_buf
        dp2.grad_ready(q)
        early = max(early, sum(dp2._launched)) if dp2._expected is not None and dp2._active else early
    dp2.finish(flat2)
    for j, sz in enumerate(sizes2):
        want = sum((r + 1) * (j + 1) + step for r in range(dp2.world))
        assert torch.all(flat2[int(offs2[j]): int(offs2[j]) + sz] == want), ("rebuilt", step, j)
    assert (early > 0) == (step >= 1), ("rebuilt", step, early)
# ... and the state the advisor described (armed on a buffer that is then retired, buckets already in flight) is refused
# loudly instead of reducing twice: every rank raises, after waiting for the handles it launched
flat2.zero_()
dp2.begin_step(opt, None, None)
for j in reversed(range(len(vs2))):
    vs2[j].grad = vs2[j].grad_buf
    dp2.grad_ready(vs2[j])
assert any(dp2._launched)
try:
    dp2.finish(torch.zeros(int(offs2[-1])))
    raise SystemExit("finish() accepted a retired buffer")
except RuntimeError as e:
    assert "gradient buffer changed" in str(e), e
dist.barrier(); dist.destroy_process_group()
print("rank", dp.rank, "ok")
'''


def test_data_parallel_allreduce_gloo_world2(tmp_path):
    """N>1 path on CPU: world_size-2 gloo process group through the same DataParallel class the GPU
    path uses with RCCL (bucketed async all-reduce of the flat gradient buffer + weight broadcast)."""
    script = tmp_path / "dp.py"
    script.write_text(_DP_SCRIPT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs)


def test_data_parallel_cuda_branch_with_fake_streams(monkeypatch):
    """The device branch of DataParallel._launch / finish (communication stream, event waits on the main and side streams,
    async handles, the join) cannot run here - there is no GPU - and on the one-GPU box it runs over a one-rank RCCL
    communicator (tests/test_dp_gpu.py).  This drives the same code with recording fakes for torch.cuda and
    torch.distributed and checks the ORDER of operations: a bucket's collective is enqueued on the communication stream only
    after that stream waits for events recorded on BOTH producer streams, nothing waits for the collective until finish(),
    and finish() waits for every handle before the current stream joins the communication stream."""
    import types
    import torch
    from boosted_detr_amd import training
    log = []

    class FakeStream:
        def __init__(self, name): self.name = name
        def wait_event(self, ev): log.append(("wait_event", self.name, ev.on))
        def wait_stream(self, other): log.append(("wait_stream", self.name, other.name))

    class FakeEvent:
        def __init__(self, enable_timing=False): self.on = None
        def record(self, st=None): self.on = (st or cur[0]).name; log.append(("record", self.on))

    class FakeCtx:
        def __init__(self, st): self.st = st
        def __enter__(self): self.prev, cur[0] = cur[0], self.st
        def __exit__(self, *a): cur[0] = self.prev

    main, side, comm = FakeStream("main"), FakeStream("side"), FakeStream("comm")
    cur = [main]
    fake_cuda = types.SimpleNamespace(Stream=lambda device=None: comm, Event=FakeEvent, stream=lambda st: FakeCtx(st),
                                      current_stream=lambda: cur[0], synchronize=lambda: None)
    monkeypatch.setattr(training.torch, "cuda", fake_cuda)

    class Handle:
        def __init__(self, n): self.n = n
        def wait(self): log.append(("handle_wait", self.n, cur[0].name))

    class FakeDist:
        class ReduceOp: SUM = "sum"; MAX = "max"
        @staticmethod
        def is_initialized(): return True
        @staticmethod
        def get_world_size(): return 2
        @staticmethod
        def get_rank(): return 0
        @staticmethod
        def all_reduce(t, op=None, async_op=False):
            log.append(("all_reduce", t.numel(), cur[0].name)); return Handle(t.numel())
    monkeypatch.setitem(sys.modules, "torch.distributed", FakeDist)
    monkeypatch.setattr(torch, "distributed", FakeDist, raising=False)

    class FlatOnDevice:                      # a flat buffer that says it lives in HBM
        is_cuda, device = True, "cuda:0"
        def __init__(self, n, base=4096): self.n, self.base = n, base
        def numel(self): return self.n
        def data_ptr(self): return self.base
        def __getitem__(self, sl): return FlatOnDevice(sl.stop - sl.start, self.base + 4 * sl.start)

    class V: pass
    flat = FlatOnDevice(2500)
    sizes, vs, off = [1200, 800, 500], [], 0
    for i, sz in enumerate(sizes):
        v = V(); v.name = f"v{i}"; v.grad_buf = flat[off: off + sz]; v.grad = v.grad_buf; v._grad_flat = flat
        vs.append(v); off += sz
    opt = types.SimpleNamespace(flat_grad=flat, vars=vs)
    dp = training.DataParallel()
    dp.BUCKET_ELEMS = 1000
    assert dp.active and dp.world == 2
    for step in range(2):                    # step 0 learns the contribution counts, step 1 launches from grad_ready
        log.clear()
        dp.begin_step(opt, main, side)
        for v in reversed(vs):
            dp.grad_ready(v)
        early = [e for e in log if e[0] == "all_reduce"]
        assert (len(early) > 0) == (step == 1), (step, log)
        assert not any(e[0] == "handle_wait" for e in log)                   # nothing waits before finish()
        dp.finish(flat)
        ar = [i for i, e in enumerate(log) if e[0] == "all_reduce"]
        assert len(ar) == 3 and all(log[i][2] == "comm" for i in ar)         # 3 buckets, all enqueued on the communication stream
        for i in ar:                                                         # ... each behind waits for main AND side
            pre = log[max(0, i - 4): i]
            assert ("wait_event", "comm", "main") in pre and ("wait_event", "comm", "side") in pre, (i, log)
        waits = [i for i, e in enumerate(log) if e[0] == "handle_wait"]
        join = log.index(("wait_stream", "main", "comm"))
        assert len(waits) == 3 and max(waits) < join and min(waits) > max(ar)
    flag = torch.zeros(1)
    dp.any_(flag)
    assert log[-1] == ("all_reduce", 1, "main")
    # bucket table at the bench's size (31.0 M gradients, 32-MB buckets): the bucket that completes LAST - the first layers', at the start
    # of the buffer - is cut to TAIL_ELEMS so that the all-reduce nothing can overlap is small (round 5)
    big = FlatOnDevice(31_006_681)
    vb = []
    for i, (o, sz) in enumerate(((0, 9408), (500_000, 147_456), (1_048_000, 4_000), (20_000_000, 2_359_296))):
        v = V(); v.name = f"b{i}"; v.grad_buf = big[o: o + sz]; v.grad = v.grad_buf; v._grad_flat = big
        vb.append(v)
    dp3 = training.DataParallel()
    dp3.prepare(types.SimpleNamespace(flat_grad=big, vars=vb))
    n, B, T = 31_006_681, dp3.BUCKET_ELEMS, dp3.TAIL_ELEMS
    assert dp3._bounds[0] == (n - B, n) and dp3._bounds[-2:] == [(T, n - 3 * B), (0, T)] and len(dp3._bounds) == 5, dp3._bounds
    assert all(a[0] == b[1] for a, b in zip(dp3._bounds[:-1], dp3._bounds[1:]))            # contiguous cover, high to low
    assert dp3._var_bucket[id(vb[0])] == (4, 4) and dp3._var_bucket[id(vb[2])] == (4, 3) and dp3._var_bucket[id(vb[3])][0] == 1      # vb[2] straddles the cut: counted in both


@pytest.mark.parametrize("good, step_ms, want", [([0, 1, 2], {0: 28.0, 1: 25.0, 2: 28.5}, 1), ([1, 3], {1: 27.0, 3: 24.9}, 3), ([2], {}, 2), ([], {}, None)])
def test_side_stream_tuning_schedule_has_a_fixed_length_and_keeps_the_fastest_candidate(monkeypatch, good, step_ms, want):
    """training.SidePlacementTuner (the data-parallel model settles between the good side-stream candidates by timing its
    first eager steps) with fakes for the engine and the events: whatever the number of good candidates, tuning ends at the SAME step - every
    rank must leave it together: the captured step and bench.py's set-up loop key on it - the first step of a slot is not counted, the
    fastest candidate is selected and the others released."""
    import types
    from boosted_detr_amd import training, engine
    clock = [0.0]
    sel, released = [], []

    class FakeEvent:
        def __init__(self, enable_timing=False): self.t = None
        def record(self): self.t = clock[0]
        def synchronize(self): pass
        def elapsed_time(self, other): return other.t - self.t
    monkeypatch.setattr(training.torch, "cuda", types.SimpleNamespace(Event=FakeEvent))
    placement = {"picked": good[0], "good": list(good)} if good else None            # None: no measured side stream (BDETR_SIDE_CANDIDATES=1, side stream off)
    monkeypatch.setattr(engine, "side_stream_placement", lambda: placement)
    monkeypatch.setattr(engine, "side_stream_expand", lambda: list(good))
    monkeypatch.setattr(engine, "side_stream_select", lambda c: (sel.append(c), placement.__setitem__("picked", c)))
    monkeypatch.setattr(engine, "side_stream_release", lambda: released.append(True))
    tuner = training.SidePlacementTuner(types.SimpleNamespace(active=True))
    first_done = None
    for step in range(30):
        pending = tuner.pending()
        tok = tuner.begin(step)
        if tok is not None and tok.begin is not None:
            clock[0] += step_ms[tok.candidate] + (7.0 if tok.rep == 0 else 0.0)       # the first step of a slot is slower (and must not count)
            tuner.mark_joined()
        tuner.end()
        if pending and not tuner.pending() and first_done is None:
            first_done = step + 1
    assert training.SidePlacementTuner(None).pending() is False                        # no data parallelism: nothing to settle
    assert first_done == training.Model.SIDE_TUNE_FROM + training.Model.SIDE_TUNE_SLOTS * training.Model.SIDE_TUNE_STEPS, first_done
    if len(good) >= 2:
        assert placement["picked"] == want and sel[-1] == want and released, (placement, sel)
        assert placement["step_ms"] == {c: step_ms[c] for c in good}, placement
    else:
        assert not sel, sel


class _GuardRig:
    """training.RangeGuard over fakes (none of this is product code): a CPU tensor as the pinned flag log, events that do nothing, a
    flag_snapshot that does on the host what bdetr_flag_snapshot does on the device, and a step that raises the flag - which then stays
    up, as on the device - for a batch marked "bad" while the owner's policy is 'split'."""

    def __init__(self, monkeypatch, **guard_attrs):
        import types
        import torch
        from boosted_detr_amd import training
        self.flag = torch.zeros(1, dtype=torch.int32)
        self.calls = []                      # (batch name, policy, use_graph, steps_done on entry) of every step

        class FakeEvent:
            def record(self): pass
            def synchronize(self): pass

        def flag_snapshot(ordinal, host):
            ordinal += 1
            host[1 + int(ordinal) % (host.numel() - 1)] = self.flag[0]
            host[0] = ordinal[0]

        def allocate(guard):
            guard.host = torch.zeros(1 + guard.RING, dtype=torch.int32)
            guard.ordinal = torch.zeros(1, dtype=torch.int32)
            guard.events = [FakeEvent() for _ in range(guard.RING)]
        monkeypatch.setattr(training.torch, "cuda", types.SimpleNamespace(Event=FakeEvent, synchronize=lambda: None))
        monkeypatch.setattr(training.K, "overflow_flag", lambda: self.flag)
        monkeypatch.setattr(training.K, "flag_snapshot", flag_snapshot)
        monkeypatch.setattr(training.RangeGuard, "_allocate", allocate)
        self.owner = types.SimpleNamespace(train_gemm_precision="split", use_graph=True, steps_done=0, optimizer=types.SimpleNamespace(iterations=0))
        self.guard = training.RangeGuard(self.owner, self.step_once)
        for k, v in guard_attrs.items():
            setattr(self.guard, k, v)

    def step_once(self, batch):
        o = self.owner
        self.calls.append((batch["name"], o.train_gemm_precision, o.use_graph, o.steps_done))
        if batch.get("bad") and o.train_gemm_precision == "split":
            self.flag[0] = 1
        self.guard.snapshot()
        o.steps_done += 1
        o.optimizer.iterations += 1
        return ("logs", batch["name"], o.train_gemm_precision)

    def train_step(self, name, bad=False, **tensors):
        batch = {"name": name, "bad": bad, **tensors}
        return self.guard.poll(batch, self.step_once(batch))


def test_range_guard_examines_an_entry_exactly_lag_steps_late_and_redoes_everything_since(monkeypatch, capsys):
    rig = _GuardRig(monkeypatch)
    g, o = rig.guard, rig.owner
    LAG = g.LAG
    assert LAG == 2 and g.flush() is None                                            # nothing pending: nothing to resolve
    for t in range(1, 4):                                                            # clean steps: entry t leaves when step t + LAG has run
        assert rig.train_step(f"b{t}") == ("logs", f"b{t}", "split")
        assert [p.ordinal for p in g.pending] == list(range(max(1, t - LAG + 1), t + 1))
    assert rig.train_step("b4", bad=True) == ("logs", "b4", "split")                 # raised here ...
    for t in range(5, 4 + LAG):
        rig.train_step(f"b{t}")
        assert g.redos == 0                                                          # ... not looked at before its turn
    n_calls = len(rig.calls)
    logs = rig.train_step(f"b{4 + LAG}")                                             # ... but exactly LAG steps later
    redone = rig.calls[n_calls + 1:]
    assert [c[0] for c in redone] == [f"b{t}" for t in range(4, 5 + LAG)]            # that batch and every later pending one
    assert all(c[1] == "mixed" and c[2] is False for c in redone)                    # on the exact-fp32 forward, eagerly
    assert redone[0][3] == 3                                                         # both counters rolled back by LAG + 1 first
    assert logs == ("logs", f"b{4 + LAG}", "mixed")                                  # the caller gets the last redone step's logs
    assert (o.steps_done, o.optimizer.iterations) == (4 + LAG, 4 + LAG)              # no batch lost, the schedule not ahead
    assert (g.redos, g.skipped, g.redo_streak) == (1, LAG + 1, 1) and not g.pending and int(rig.flag) == 0
    assert (o.train_gemm_precision, o.use_graph) == ("split", True)                  # both restored behind the redo
    err = capsys.readouterr().err
    assert err == ("[boosted_detr_amd] step 3: the split-fp16 forward left its range (|x| >= 65504) or went non-finite; "
                   f"no update was applied since - redoing {LAG + 1} batch(es) on the exact-fp32 forward\n")
    rig.train_step("c1"), rig.train_step("c2", bad=True)
    assert [p.ordinal for p in g.pending] == [g.launched - 1, g.launched] and g.redos == 1
    assert g.flush() == ("logs", "c2", "mixed") and g.redos == 2 and g.skipped == LAG + 2      # flush: the clean one passes, the raised one is redone
    assert g.flush() is None and not g.pending


def test_range_guard_ring_index_wraps(monkeypatch):
    rig = _GuardRig(monkeypatch)
    g = rig.guard
    RING = g.RING
    for t in range(1, 2 * RING + 2):
        rig.train_step(f"b{t}", bad=(t == RING + 1))                                 # its flag lands in ring entry (RING + 1) % RING = 1
        assert g.launched == t and (not g.pending or g.pending[-1].event is g.events[t % RING])
        assert g.redos == (1 if t >= RING + 1 + g.LAG else 0), t
    assert int(g.host[0]) == g.launched == 2 * RING + 1                              # (the redone steps ran under 'mixed': unguarded, no snapshot)
    # the raised entry of step RING + 1 has been overwritten by step 2 RING + 1's clean one; the LAG attempts behind it (flag still up) not yet
    assert rig.owner.steps_done == 2 * RING + 1 and g.host[1:].tolist() == [int(2 <= i <= 1 + g.LAG) for i in range(RING)]


def test_range_guard_refuses_to_redo_a_batch_modified_in_place(monkeypatch):
    import torch
    rig = _GuardRig(monkeypatch)
    image, boxes = torch.zeros(4), torch.zeros(4)
    rig.train_step("b1", bad=True, image=image, bbox=boxes)
    image.add_(1.0)                                                                  # an input pipeline reusing its buffer
    rig.train_step("b2")
    with pytest.raises(RuntimeError, match=r"step ordinal 1 must be redone, but its tensors \['image'\] were modified in place"):
        rig.train_step("b3")


def test_range_guard_demotes_after_consecutive_redos_only(monkeypatch, capsys):
    rig = _GuardRig(monkeypatch, resolve_at_once=True)
    g, o = rig.guard, rig.owner
    assert g.DEMOTE_AFTER == 3
    for i, bad in enumerate([True, True, False, True, True]):                        # a clean step in between resets the streak
        rig.train_step(f"b{i}", bad=bad)
    assert (g.redos, g.redo_streak, o.train_gemm_precision) == (4, 2, "split")
    assert "consecutive" not in capsys.readouterr().err
    rig.train_step("b5", bad=True)
    assert (g.redos, g.redo_streak, o.train_gemm_precision) == (5, 3, "mixed")       # for good ...
    assert capsys.readouterr().err.endswith(
        "[boosted_detr_amd] 3 consecutive range-guard redos: train_gemm_precision is now 'mixed' (exact-fp32 forward) "
        "for the rest of this model's life; set it back to 'split' by hand if the cause was transient\n")
    n = len(rig.calls)
    assert rig.train_step("b6", bad=True) == ("logs", "b6", "mixed") and len(rig.calls) == n + 1 and g.redos == 5      # ... and the guard is off
    assert (o.steps_done, o.optimizer.iterations) == (7, 7)


def test_every_kernel_switch_is_forced_by_some_test():
    """Each getenv("BDETR_...") in csrc/*.hip selects a compiled variant or a code path: every name must be set by some test (the
    forced-variant children of tests/test_variants_gpu.py, mostly) or be listed here with the reason it needs none.  A new A/B
    switch fails this test until a test forces it."""
    import glob
    import re
    needs_no_variant_test = {
        "BDETR_SGEMM_DBG": "diagnostic builds only (compiled under BDETR_SGEMM_DIAG)",
        "BDETR_GEMM_PRECISION": "initial value of the policy word every precision test sets through bdetr_set_gemm_precision",
        "BDETR_WGRAD_WANT": "split-K occupancy target: changes the slice count, no kernel",
        "BDETR_WGRAD_WANT_3X3": "split-K occupancy target of the im2col layers: no kernel",
        "BDETR_WGRAD_WANT_64": "split-K occupancy target of the 64x64 3x3 layers: no kernel",
        "BDETR_WGRAD_MINSTAGES": "lower bound of K-steps per split-K slice: no kernel",
        "BDETR_ZERO_MEMSET": "set by tests/test_training_gpu.py (hipMemsetAsync instead of the zero kernel)",
    }
    names = set()
    for path in glob.glob(os.path.join(ROOT, "boosted_detr_amd", "csrc", "*.hip")):
        with open(path) as f:
            names |= set(re.findall(r'getenv\("(BDETR_[A-Z0-9_]+)"\)', f.read()))
    assert len(names) >= 13, sorted(names)                      # the scan itself still finds the switches
    tests = ""
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        if os.path.basename(path) != "test_host_cpu.py":
            with open(path) as f:
                tests += f.read()
    forced = {n for n in names if re.search(r'["\']%s["\']\s*:|\b%s\s*=' % (n, n), tests)}
    stale = sorted(set(needs_no_variant_test) - names)
    assert not stale, f"allow-list entries without a getenv in csrc: {stale}"
    missing = sorted(names - forced - set(needs_no_variant_test))
    assert not missing, f"kernel switches no test forces: {missing}"


def test_every_included_header_is_a_build_dependency():
    """build() decides what to recompile from a digest of its sources and build.headers(): a header that a translation unit
    includes but the list misses would never trigger a rebuild.  Every #include "x.h" in csrc/* must resolve to a listed file."""
    import re
    from boosted_detr_amd import build
    listed = {p.resolve() for p in build.headers()}
    assert all(p.is_file() for p in listed), sorted(str(p) for p in listed if not p.is_file())
    includes = []
    for path in sorted(build.CSRC.iterdir()):
        if path.suffix in (".h", ".hip", ".cpp"):
            includes += [(path.name, inc) for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', path.read_text(), flags=re.M)]
    assert len(includes) >= len(build.SOURCES), includes         # the scan itself still finds the includes
    missing = sorted((src, inc) for src, inc in includes if (build.CSRC / inc).resolve() not in listed)
    assert not missing, f"headers included but not in build.headers(): {missing}"
