"""GPU tests of training.AdamW: the fused multi-tensor kernel (bdetr_adamw_clipnorm) against the fp64 restatement of
tests/_adamw_ref.py, the skip-flag contract, the optimizer through compile / fit, graph replay, freeze -> unfreeze, checkpoints with
optimizer slots (AdamW and SGD), one data-parallel step, and the SGD entry point's bits against digests recorded from the build
before sqnorm_kernel took its table stride as an argument.

Tolerance rule of the kernel comparisons (no fixed number): next to the fp64 restatement runs a NumPy fp32 restatement in the op
order include/bdetr.h documents; per tensor and per quantity the kernel's max error against fp64 may be at most 4 x the fp32
restatement's max error against fp64, plus one ulp of the tensor's max magnitude (the floor for cases where the restatement is exact).
4 x is the project's margin for "fp32 code vs fp32 oracle".  Measured on MI355X: see profiles/README.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _adamw_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_model(**kw):
    from boosted_detr_amd import parameters, transformers
    from boosted_detr_amd.model import DETR
    transformers.AttentionBlock.dropout_rate = kw.pop("dropout", 0.0)
    transformers.FeedForwardBlock.dropout_rate = transformers.AttentionBlock.dropout_rate
    return DETR(num_object_preds=10, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256,
                num_decoder_blocks=2, num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32,
                vocab_dict=parameters.synthetic_vocab(10, 4), attribute_weight=1.0, **kw)


def small_batch(seed=9, B=2):
    from oracle import detr_oracle as O
    cfg = O.Config(image_size=(64, 64), num_object_preds=10, num_decoder_blocks=2, num_categories=12, num_attributes=6)
    return cfg, O.make_batch(cfg, B, 5, seed=seed, num_objects=[2, 4][:B])


def device_batch(host):
    from boosted_detr_amd.engine import to_device
    return {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
            "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}


@pytest.fixture
def deterministic():
    """BDETR_DETERMINISTIC mode for one test (what test_training_gpu.py's fixture of this name sets): no float atomics, two runs of
    one step give bit-identical weights."""
    from boosted_detr_amd import kernels as K
    prev = K.set_deterministic(True)
    yield
    K.set_deterministic(prev)


def host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().ravel().copy()


def check_against_restatements(label, got, ref64, ref32, ratios):
    """The tolerance rule of this file's docstring for one tensor and one quantity; records kernel error / allowance."""
    got = got.astype(np.float64)
    err_k = float(np.abs(got - ref64).max())
    err_r = float(np.abs(ref32.astype(np.float64) - ref64).max())
    floor = float(np.spacing(np.float32(np.abs(ref64).max())))
    ratios[label] = max(ratios.get(label, 0.0), err_k / (err_r + floor / 4))
    assert err_k <= 4 * err_r + floor, (label, err_k, err_r, floor)


def _snapshot(opt):
    return [[t.clone() for t in ts] for ts in ([v.value for v in opt.vars], opt.m_views, opt.v_views)]


def _identical(before, opt) -> bool:
    return all(torch.equal(a, b) for old, new in zip(before, ([v.value for v in opt.vars], opt.m_views, opt.v_views)) for a, b in zip(old, new))


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. the kernel against fp64 on synthetic tensors that hit every path
# ----------------------------------------------------------------------------------------------------------------------------------
def test_adamw_kernel_matches_fp64_restatement_on_every_path(cuda):
    from boosted_detr_amd.training import AdamW
    lr, wd = 1e-3, 1e-2
    vs = R.make_variables(R.seeded_weights())
    opt = AdamW(lr, weight_decay=wd, clipnorm=R.CLIPNORM, exclude_from_weight_decay=R.EXCLUDE)
    opt.build(vs)
    assert [opt.decays(v.name) for v in vs] == [i != R.NO_DECAY_INDEX for i in range(len(vs))]
    assert vs[R.OFFSET_INDEX].value.data_ptr() % 16 == 4 and all(g.data_ptr() % 16 == 0 for g in opt.grad_views)
    w = [host(v.value) for v in vs]
    m = [np.zeros_like(x) for x in w]
    v_ = [np.zeros_like(x) for x in w]
    ratios, clipped, unclipped = {}, set(), set()
    for step in range(20):
        gs = R.seeded_gradients(step)
        assert any((g == 0).any() for g in gs)
        for gv, g in zip(opt.grad_views, gs):
            gv.copy_(torch.from_numpy(g).to(gv.device))
        opt.apply_gradients()
        torch.cuda.synchronize()
        assert opt.iterations == step + 1
        for i, var in enumerate(vs):
            decay = i != R.NO_DECAY_INDEX
            kw = dict(lr=lr, wd=wd, t=step + 1, clipnorm=R.CLIPNORM, decay=decay)
            (clipped if float(np.linalg.norm(gs[i].astype(np.float64))) > R.CLIPNORM else unclipped).add(i)
            ref64 = R.adamw_step64(w[i], gs[i], m[i], v_[i], **kw)
            ref32 = R.adamw_step32(w[i], gs[i], m[i], v_[i], **kw)
            got = (host(var.value), host(opt.m_views[i]), host(opt.v_views[i]))
            for q, a, b, c in zip("wmv", got, ref64, ref32):
                check_against_restatements(f"{q}[{R.SIZES[i]}]", a, b, c, ratios)
            # decoupled weight decay is visible where it applies and absent where the variable is excluded
            nodecay64 = R.adamw_step64(w[i], gs[i], m[i], v_[i], **dict(kw, decay=False))[0]
            differs = float(np.abs(got[0] - nodecay64).max()) > 1e-2 * wd * float(np.abs(w[i]).max())
            assert differs == decay, (var.name, step)
            w[i], m[i], v_[i] = got                   # the next step's reference starts from the kernel's state: rounding does not compound
    assert clipped and unclipped and R.NO_DECAY_INDEX in clipped, (clipped, unclipped)
    worst = max(ratios, key=ratios.get)
    print("kernel error / (fp32 restatement's error + ulp/4), allowance 4; worst:", worst, round(ratios[worst], 3),
          "| per quantity:", {q: round(max(r for k, r in ratios.items() if k[0] == q), 3) for q in "wmv"})


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. the skip flag
# ----------------------------------------------------------------------------------------------------------------------------------
def test_skip_flag_and_non_finite_gradient_leave_w_m_v_untouched(cuda):
    from boosted_detr_amd.training import AdamW
    vs = R.make_variables(R.seeded_weights())
    opt = AdamW(1e-3, weight_decay=1e-2, clipnorm=R.CLIPNORM)
    opt.build(vs)

    def load(step):
        for gv, g in zip(opt.grad_views, R.seeded_gradients(step)):
            gv.copy_(torch.from_numpy(g).to(gv.device))

    load(0)
    opt.apply_gradients()                                  # one applied step: non-zero m and v
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) > 0 for t in opt.m_views[1:]) and opt.iterations == 1
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    before = _snapshot(opt)
    load(1)
    opt.apply_gradients(skip_flag=flag)                    # raised beforehand: nothing moves
    torch.cuda.synchronize()
    assert int(flag.item()) == 1 and _identical(before, opt)
    flag.zero_()
    opt.flat_grad[opt.flat_grad.numel() // 2] = float("nan")      # a value in a buffer (inside the ~2 M-element tensor)
    opt.apply_gradients(skip_flag=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1                           # the norm pass raised it ...
    assert _identical(before, opt)                         # ... and no tensor was touched, not even those with a clean gradient
    # like SGD.apply_gradients, the call counts an iteration whether or not the device applied it: the host side of the range guard
    # (RangeGuard.redo) rolls `iterations` back for update-free attempts, and with it Adam's bias correction
    assert opt.iterations == 3
    opt.iterations = 1
    flag.zero_()
    load(1)
    opt.apply_gradients(skip_flag=flag)                    # a clean gradient goes through
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and opt.iterations == 2
    assert not any(torch.equal(a, v.value) for a, v in zip(before[0], opt.vars))


# ----------------------------------------------------------------------------------------------------------------------------------
# 12. the SGD entry point did not change its bits
# ----------------------------------------------------------------------------------------------------------------------------------
def test_sgd_entry_point_reproduces_the_digests_of_the_build_before_the_stride_argument(cuda):
    with open(os.path.join(ROOT, "tests", "golden", "sgd_parent_digests.json")) as f:
        want = json.load(f)
    got = R.sgd_digests()
    assert got["inputs"] == want["inputs"], "the seeded inputs differ from the recorded ones (NumPy's generator?): nothing to compare"
    assert got["steps"] == want["steps"]


# ----------------------------------------------------------------------------------------------------------------------------------
# 7. through the model
# ----------------------------------------------------------------------------------------------------------------------------------
def test_adamw_through_the_model_matches_restatement_and_fit_trains(cuda):
    from boosted_detr_amd.training import AdamW, TerminateOnNaN
    from oracle import detr_oracle as O
    cfg, batch = small_batch()
    model = small_model()
    opt = AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1)              # the notebook's line (cell 26)
    model.compile(optimizer=opt)
    model.forward_backward(batch)                                   # build
    model.set_weights_dict(O.make_params(cfg, seed=1))
    tv = model.trainable_variables
    w = {v.name: host(v.value) for v in tv}
    m = {k: np.zeros_like(x) for k, x in w.items()}
    v_ = {k: np.zeros_like(x) for k, x in w.items()}
    ratios = {}
    for step in range(2):
        model.forward_backward(batch)
        opt.stage_gradients(tv)
        g = {v.name: host(v.grad) for v in tv}
        opt.apply_gradients()
        torch.cuda.synchronize()
        for i, var in enumerate(opt.vars):
            k = var.name
            kw = dict(lr=1e-4, wd=1e-3, t=step + 1, clipnorm=0.1)
            ref64 = R.adamw_step64(w[k], g[k], m[k], v_[k], **kw)
            ref32 = R.adamw_step32(w[k], g[k], m[k], v_[k], **kw)
            got = (host(var.value), host(opt.m_views[i]), host(opt.v_views[i]))
            for q, a, b, c in zip("wmv", got, ref64, ref32):
                check_against_restatements(f"{q}:{k}", a, b, c, ratios)
            w[k], m[k], v_[k] = got
    assert opt.iterations == 2 and len(opt.vars) == len(tv) > 100
    worst = max(ratios, key=ratios.get)
    print("through the model, kernel error / allowance base (allowance 4); worst:", worst, round(ratios[worst], 3))

    model = small_model(dropout=0.0)
    model.compile(optimizer=AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1))
    hist = model.fit([batch] * 8, epochs=3, validation_data=[batch], callbacks=[TerminateOnNaN()], verbose=0)
    print("fit() epoch losses:", hist["loss"])
    assert len(hist["loss"]) == 3 and all(np.isfinite(hist["loss"])) and not model.stop_training
    assert hist["loss"][2] < hist["loss"][0]
    assert model.optimizer.iterations == 27                          # 3 x (8 + 1): test_step also trains (model.py:235-236)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8. graph replay equals eager
# ----------------------------------------------------------------------------------------------------------------------------------
def _slots(m):
    opt = m.optimizer
    return {f"{slot}/{v.name}": host(t) for slot in opt.slot_views for v, t in zip(opt.vars, opt.slot_views[slot])}


def _differing(a: dict, b: dict):
    assert a.keys() == b.keys()
    return [k for k in a if not np.array_equal(a[k], b[k])]


def test_graph_replayed_adamw_steps_equal_eager_steps(cuda, deterministic):
    """Six steps eager against the same six with use_graph (two eager warm-ups, the capture, replays): weights, m and v bit-identical.
    lr_t carries the bias correction of step t and changes every step even at a constant learning rate: a value baked into the
    captured segment on the host would fail this."""
    from boosted_detr_amd.training import AdamW, CosineDecayRestarts
    from oracle import detr_oracle as O
    cfg, hb = small_batch()
    params = O.make_params(cfg, seed=1)
    batches = [device_batch(hb), device_batch(small_batch(seed=21)[1])]
    runs = {}
    for graph in (False, True):
        m = small_model(dropout=0.1)
        m.compile(optimizer=AdamW(CosineDecayRestarts(1e-4, 10, m_mul=.95, alpha=.1), weight_decay=lambda it: 1e-3 / (1 + it), clipnorm=.1))
        m.forward_backward(batches[0])
        m.set_weights_dict(params)
        m.use_graph = graph
        losses = [m.logs_to_host(m.train_step(batches[i % 2]))["loss"] for i in range(6)]
        assert (len(m._graphs) == 1) == graph and m.steps_done == 6 and m.optimizer.iterations == 6
        runs[graph] = (losses, m.get_weights_dict(), _slots(m))
    assert all(np.isfinite(runs[True][0])) and runs[False][0] == runs[True][0], (runs[False][0], runs[True][0])
    assert not _differing(runs[False][1], runs[True][1]), _differing(runs[False][1], runs[True][1])[:5]
    assert not _differing(runs[False][2], runs[True][2]), _differing(runs[False][2], runs[True][2])[:5]
    assert any(np.abs(x).max() > 0 for k, x in runs[True][2].items() if k.startswith("v/"))


# ----------------------------------------------------------------------------------------------------------------------------------
# 9. freeze -> unfreeze keeps m and v; changed hyper-parameters do not replay an old capture
# ----------------------------------------------------------------------------------------------------------------------------------
def test_moments_survive_a_freeze_unfreeze_cycle(cuda):
    from boosted_detr_amd.training import AdamW
    cfg, batch = small_batch()
    m = small_model()
    m.compile(optimizer=AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1))
    for _ in range(2):
        m.train_step(batch)
    opt = m.optimizer
    stay = m.CategoryPredictionHead.DenseOut.kernel
    i = [id(x) for x in opt.vars].index(id(stay))
    keep = (opt.m_views[i].clone(), opt.v_views[i].clone())
    fz = next(x for x in opt.vars if x.name.startswith(m.EncoderBackbone.scope))
    k = [id(x) for x in opt.vars].index(id(fz))
    at_freeze = (opt.m_views[k].clone(), opt.v_views[k].clone())
    assert float(at_freeze[1].abs().max()) > 0
    m.EncoderBackbone.trainable = False
    m.forward_backward(batch)                                          # rebuilds the flat buffers for the smaller set
    j = [id(x) for x in opt.vars].index(id(stay))
    assert len(opt.vars) < 200 and torch.equal(opt.m_views[j], keep[0]) and torch.equal(opt.v_views[j], keep[1])
    assert torch.equal(fz._adam_m, at_freeze[0]) and torch.equal(fz._adam_v, at_freeze[1])
    m.EncoderBackbone.trainable = True
    m.forward_backward(batch)
    k = [id(x) for x in opt.vars].index(id(fz))
    assert torch.equal(opt.m_views[k], at_freeze[0]) and torch.equal(opt.v_views[k], at_freeze[1])
    assert fz._adam_m is None and fz._adam_v is None


def test_changed_beta_2_does_not_replay_the_old_capture(cuda):
    from boosted_detr_amd.training import AdamW
    cfg, hb = small_batch()
    batch = device_batch(hb)
    m = small_model()
    m.compile(optimizer=AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1))
    m.use_graph = True
    for _ in range(4):
        m.train_step(batch)
    assert len(m._graphs) == 1
    m.optimizer.beta_2 = 0.99                                          # a by-value kernel argument of the captured segment
    for _ in range(4):
        m.train_step(batch)
    assert len(m._graphs) == 2                                         # a fresh capture for the new hyper-parameters
    m.compile(optimizer=AdamW(1e-4, beta_2=0.98, weight_decay=1e-3, clipnorm=0.1))
    assert not m._graphs                                               # a new optimizer retires every captured step
    for _ in range(4):                                                 # (the first step builds the new optimizer's buffers: a signature of its own)
        logs = m.logs_to_host(m.train_step(batch))
    assert np.isfinite(logs["loss"]) and len(m._graphs) == 1 and m.optimizer.iterations == 4


# ----------------------------------------------------------------------------------------------------------------------------------
# 10. resume from a checkpoint with optimizer slots
# ----------------------------------------------------------------------------------------------------------------------------------
def _make_optimizer(kind):
    from boosted_detr_amd.training import SGD, AdamW, CosineDecayRestarts
    if kind == "adamw":
        return AdamW(CosineDecayRestarts(1e-4, 10, m_mul=.95, alpha=.1), weight_decay=1e-3, clipnorm=.1)
    return SGD(CosineDecayRestarts(1e-3, 10, m_mul=.95, alpha=.1), momentum=.9, nesterov=True, clipnorm=.1)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_resume_with_optimizer_slots_continues_the_run_bit_for_bit(cuda, deterministic, tmp_path, kind):
    from oracle import detr_oracle as O
    from safetensors.numpy import load_file
    cfg, hb = small_batch()
    batch = device_batch(hb)
    params = O.make_params(cfg, seed=1)
    a = small_model(dropout=0.1)
    a.compile(optimizer=_make_optimizer(kind))
    a.forward_backward(batch)
    a.set_weights_dict(params)
    for _ in range(4):
        a.train_step(batch)
    path, plain = str(tmp_path / "with_slots"), str(tmp_path / "plain")
    a.save_weights(path, include_optimizer=True)
    a.save_weights(plain)
    nslots = len(a.optimizer.SLOTS)
    stored = load_file(path + ".safetensors")
    assert sum(k.startswith("optimizer_slot/") for k in stored) == nslots * len(a.optimizer.vars)
    assert not any(k.startswith("optimizer_slot/") for k in load_file(plain + ".safetensors"))
    for _ in range(4):
        a.train_step(batch)
    a.guard_flush(); torch.cuda.synchronize()

    def resumed(file):
        b = small_model(dropout=0.1)
        b.compile(optimizer=_make_optimizer(kind))
        b.train_step(batch)                                            # build: variables, flat buffers, slots
        b.load_weights(file)
        return b

    b = resumed(path)
    assert b.optimizer.iterations == 4 and b.steps_done == 4
    for _ in range(4):
        b.train_step(batch)
    b.guard_flush(); torch.cuda.synchronize()
    assert a.range_redos == 0 and b.range_redos == 0
    assert a.optimizer.iterations == b.optimizer.iterations == 8
    assert not _differing(a.get_weights_dict(), b.get_weights_dict()), _differing(a.get_weights_dict(), b.get_weights_dict())[:5]
    assert not _differing(_slots(a), _slots(b)), _differing(_slots(a), _slots(b))[:5]
    # a file written without the flag still loads, and leaves the slots of a fresh optimizer at zero (the behaviour before slots)
    c = small_model(dropout=0.1)
    c.compile(optimizer=_make_optimizer(kind))
    c(batch, training=False)                                           # build-by-first-call in inference mode: no optimizer state yet
    c.load_weights(plain)
    assert c.optimizer.iterations == 4
    c.forward_backward(batch)
    c.optimizer.stage_gradients(c.trainable_variables)                 # builds the slots
    assert all(float(t.abs().max()) == 0 for views in c.optimizer.slot_views.values() for t in views)


def test_slots_of_frozen_variables_are_saved_from_their_parked_copies(cuda, tmp_path):
    from boosted_detr_amd.training import AdamW, ModelCheckpoint
    from safetensors.numpy import load_file
    cfg, batch = small_batch()
    m = small_model()
    m.compile(optimizer=AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1))
    for _ in range(2):
        m.train_step(batch)
    full = m.optimizer.get_state(m.variables)
    m.EncoderBackbone.trainable = False
    m.train_step(batch)                                                # the backbone's moments are parked on its variables now
    cb = ModelCheckpoint(str(tmp_path / "full_{epoch:02d}"), save_weights_only=False)      # Keras: the full model, optimizer included
    cb.set_model(m)
    cb.on_epoch_end(0)
    stored = load_file(str(tmp_path / "full_01.safetensors"))
    frozen = [v for v in m.EncoderBackbone.variables if v.trainable]
    assert len(frozen) > 50
    for v in frozen:
        for slot in ("m", "v"):
            key = f"optimizer_slot/{slot}/{v.name}"
            assert np.array_equal(stored[key], full[key]), key         # frozen since: exactly the values at the freeze
    assert set(k for k in stored if k.startswith("optimizer_slot/")) == set(full)
    # ... and a model that loads the file while the backbone is frozen gets them back at the unfreeze
    other = small_model()
    other.compile(optimizer=AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1))
    other.train_step(batch)
    other.EncoderBackbone.trainable = False
    other.train_step(batch)
    other.load_weights(str(tmp_path / "full_01"))
    other.EncoderBackbone.trainable = True
    other.forward_backward(batch)
    got = other.optimizer.get_state()
    for v in frozen:
        assert np.array_equal(got[f"optimizer_slot/v/{v.name}"], full[f"optimizer_slot/v/{v.name}"]), v.name


# ----------------------------------------------------------------------------------------------------------------------------------
# 11. data parallel, one process: a one-rank RCCL communicator (the pattern of tests/test_dp_gpu.py, in a worker of its own)
# ----------------------------------------------------------------------------------------------------------------------------------
_WORKER_DP = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import boosted_detr_amd
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from test_adamw_gpu import small_model, small_batch, device_batch, _slots, _differing
from boosted_detr_amd import kernels as K
from boosted_detr_amd.training import AdamW, DataParallel
from oracle import detr_oracle as O
K.set_deterministic(True)
DataParallel.BUCKET_ELEMS = 1 << 19                       # several buckets on this toy (2 MB each)
cfg, hb = small_batch()
params = O.make_params(cfg, seed=1)
batch = device_batch(hb)
runs = {}
for dp in (False, True):
    m = small_model(dropout=0.1)
    m.compile(optimizer=AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1))
    m.forward_backward(batch)
    m.set_weights_dict(params)
    if dp:
        m.distribute()
        assert m._dp.active and m._dp.world == 1
    # step 1 builds the flat buffers, step 2 calibrates the bucket table, step 3 overlaps the bucket all-reduces with the backward pass
    losses = [m.logs_to_host(m.train_step(batch))["loss"] for _ in range(3)]
    m.guard_flush(); torch.cuda.synchronize()
    if dp:
        assert m._dp._expected is not None and len(m._dp._bounds) >= 3 and m._dp._flat is m.optimizer.flat_grad
    runs[dp] = (losses, m.get_weights_dict(), _slots(m), m.optimizer.iterations)
assert runs[False][0] == runs[True][0] and runs[False][3] == runs[True][3] == 3, (runs[False][0], runs[True][0])
assert not _differing(runs[False][1], runs[True][1]) and not _differing(runs[False][2], runs[True][2])
print("ADAMW_DP_OK", runs[True][0])
dist.destroy_process_group()
'''


def test_data_parallel_adamw_step_on_a_one_rank_group_equals_the_undistributed_step(cuda, deterministic, tmp_path):
    from boosted_detr_amd.training import AdamW
    # the layout DataParallel.prepare relies on: 16-byte-aligned slots, one view per variable, v.grad_buf aliasing the flat buffer
    vs = R.make_variables(R.seeded_weights())
    opt = AdamW(1e-3, weight_decay=1e-2)
    opt.build(vs)
    base = opt.flat_grad.data_ptr()
    assert len(opt.grad_views) == len(opt.vars) == len(vs)
    for v, gv in zip(opt.vars, opt.grad_views):
        assert v.grad_buf is gv and v._grad_flat is opt.flat_grad and gv.data_ptr() % 16 == 0
        assert base <= gv.data_ptr() and gv.data_ptr() + 4 * gv.numel() <= base + 4 * opt.flat_grad.numel()
    script = tmp_path / "adamw_dp.py"
    script.write_text(_WORKER_DP)
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", BDETR_DP_FORCE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0", BDETR_SIDE_TUNE="0")
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "ADAMW_DP_OK" in p.stdout, p.stdout[-3000:]
    print(p.stdout.strip().splitlines()[-1])
