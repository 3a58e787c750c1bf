"""GPU tests of the compile/fit sliver: fused SGD-Nesterov/clipnorm kernel vs the oracle's restatement of
the Keras update, fit() with callbacks, save/load round trip, layer freezing (S18)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def test_sgd_nesterov_clipnorm_matches_keras_restatement(cuda):
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg, batch = small_batch()
    model = small_model()
    opt = SGD(learning_rate=0.05, momentum=0.9, nesterov=True, clipnorm=0.1)
    model.compile(optimizer=opt)
    model.forward_backward(batch)                      # build
    model.set_weights_dict(O.make_params(cfg, seed=1))
    w0 = {v.name: v.value.detach().cpu().numpy().copy() for v in model.trainable_variables}
    vel = {k: np.zeros_like(v) for k, v in w0.items()}
    for step in range(2):
        model.forward_backward(batch)
        tv = model.trainable_variables
        opt.stage_gradients(tv)
        g = {v.name: v.grad.detach().cpu().numpy().copy() for v in tv}
        opt.apply_gradients()
        torch.cuda.synchronize()
        for v in tv:
            w_ref, v_ref = O.sgd_nesterov_clipnorm(w0[v.name].ravel(), g[v.name].ravel(), vel[v.name].ravel(), lr=0.05)
            got = v.value.detach().cpu().numpy().ravel()
            scale = np.abs(w_ref).max() + 1e-12
            assert np.abs(got - w_ref).max() <= 2e-6 * scale + 1e-7, (v.name, step)
            w0[v.name], vel[v.name] = got.reshape(w0[v.name].shape).copy(), v_ref.reshape(w0[v.name].shape)
    assert opt.iterations == 2


def test_fit_callbacks_save_load(cuda, tmp_path):
    from boosted_detr_amd.training import SGD, CosineDecayRestarts, ModelCheckpoint, TerminateOnNaN, TensorBoard, latest_checkpoint
    cfg, batch = small_batch()
    model = small_model(dropout=0.0)       # dropout noise on a 2-image toy batch is larger than one epoch's descent
    model.compile(optimizer=SGD(CosineDecayRestarts(1e-3, 4000, m_mul=.95, alpha=.1), momentum=.9, nesterov=True, clipnorm=.1))
    ckpt = str(tmp_path / "ckpt" / "weights_{epoch:02d}")
    # 3 epochs x 8 steps: single steps of this 2-image toy problem are noisy (split-K atomics make runs differ in the
    # last bits and the trajectory amplifies them), the epoch means over 8 steps are not
    hist = model.fit([batch] * 8, epochs=3, validation_data=[batch],
                     callbacks=[ModelCheckpoint(ckpt, save_weights_only=True), TerminateOnNaN(), TensorBoard(str(tmp_path / "logs"))], verbose=0)
    assert len(hist["loss"]) == 3 and all(np.isfinite(hist["loss"]))
    assert hist["loss"][2] < hist["loss"][0]                      # it trains
    assert model.optimizer.iterations == 3 * (8 + 1)               # test_step also trains (model.py:235-236)
    path = latest_checkpoint(str(tmp_path / "ckpt"))
    assert path is not None and os.path.exists(path)
    before = model.get_weights_dict()
    other = small_model()
    other(batch, training=False)                                   # build-by-first-call in inference mode
    other.load_weights(path)
    after = other.get_weights_dict()
    assert set(before) == set(after)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    cat, att, box = other({"image": batch["image"]}, training=False)
    assert cat.shape == (2, 10, 1) and box.shape == (2, 10, 4)
    assert (tmp_path / "logs" / "scalars.jsonl").exists()


def test_invalid_costs_raise_like_scipy_and_terminate_on_nan(cuda):
    """NaN targets give a NaN cost row: scipy raises ValueError inside the reference's numpy_function;
    fit() reproduces that.  TerminateOnNaN itself is a host-side callback."""
    from boosted_detr_amd.training import SGD, TerminateOnNaN
    cfg, batch = small_batch()
    model = small_model()
    model.compile(optimizer=SGD(1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    bad = dict(batch)
    bad["bbox"] = batch["bbox"].copy()
    bad["bbox"][0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        model.fit([bad, batch], epochs=1, callbacks=[TerminateOnNaN()], verbose=0)
    cb = TerminateOnNaN()
    cb.set_model(model)
    model.stop_training = False
    cb.on_batch_end(0, {"loss": 1.0})
    assert not model.stop_training
    cb.on_batch_end(1, {"loss": float("nan")})
    assert model.stop_training


def test_frozen_backbone_uses_moving_statistics_and_skips_its_gradients(cuda):
    """Boosted_DETR_COCO.ipynb cell 30: EncoderBackbone.trainable = False -> inference-mode BN (S18)."""
    from oracle import detr_oracle as O
    cfg, batch = small_batch()
    params = O.make_params(cfg, seed=2)
    model = small_model()
    model.forward_backward(batch)
    model.set_weights_dict(params)
    for layer in (model.EncoderBackbone, model.BackboneNeck, model.CategoryPredictionHead, model.AttributePredictionHead, model.BoxPredictionHead):
        layer.trainable = False
    y = model.forward_backward(batch)
    out, grads = O.train_step_grads(cfg, params, batch, dtype=torch.float64, frozen_bn=True)
    for got, want in zip(y, (out.cat_preds, out.attribute_preds, out.box_preds)):
        g, w = got.cpu().numpy().astype(np.float64), want.detach().numpy()
        assert np.abs(g - w).max() <= 1e-3 * np.abs(w).max()
    after = model.get_weights_dict()
    for k, v in params.items():
        if "moving_" in k:
            assert np.array_equal(after[k], v), k                  # frozen BN does not update its statistics
    for v in model.variables:
        if v.name.startswith(("EncoderBackbone", "BackboneNeck", "CategoryPredictionHead", "AttributePredictionHead", "BoxPredictionHead")):
            assert v.grad is None, v.name
        elif v.trainable:
            want = grads[v.name].astype(np.float64)
            if np.abs(want).max() < 1e-9:
                continue
            err = np.linalg.norm(v.grad_numpy().astype(np.float64) - want) / np.linalg.norm(want)
            assert err < 2e-2, (v.name, err)
    assert len(model.trainable_variables) < len([v for v in model.variables if v.trainable])


def test_direct_gradient_sinks_equal_staged_gradients(cuda):
    """Once the optimizer owns a flat gradient buffer the backward kernels write parameter gradients
    straight into it (ops.GradSink 'direct', split-K atomics into the pre-zeroed buffer).  One step in
    that mode must give the same gradients as the temporary-tensor path used before the optimizer is built."""
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg, batch = small_batch()
    model = small_model()
    model.compile(optimizer=SGD(1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    model.forward_backward(batch)
    model.set_weights_dict(O.make_params(cfg, seed=4))
    model.forward_backward(batch)                                   # temp path: no grad_buf yet
    staged = {v.name: v.grad.detach().cpu().numpy().copy() for v in model.trainable_variables}
    model.optimizer.stage_gradients(model.trainable_variables)      # builds the flat buffer
    model.forward_backward(batch)                                   # direct path
    assert all(v.grad is v.grad_buf for v in model.trainable_variables)
    for v in model.trainable_variables:
        a, b = v.grad.detach().cpu().numpy().astype(np.float64), staged[v.name].astype(np.float64)
        if np.abs(b).max() < 1e-7:
            assert np.abs(a).max() < 1e-7, v.name
            continue
        assert np.linalg.norm(a - b) <= 1e-5 * np.linalg.norm(b), v.name


def test_dropout_is_seeded_and_changes_per_step(cuda):
    cfg, batch = small_batch()
    model = small_model(dropout=0.1)
    a = [t.cpu().numpy() for t in model.forward_backward(batch)]
    b = [t.cpu().numpy() for t in model.forward_backward(batch)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))         # same step counter -> same masks
    model.steps_done += 1
    c = [t.cpu().numpy() for t in model.forward_backward(batch)]
    assert not np.array_equal(a[0], c[0])


def _grads_after_one_step(model, batch):
    model.forward_backward(batch)
    tv = model.trainable_variables
    model.optimizer.stage_gradients(tv)
    torch.cuda.synchronize()
    return {v.name: v.grad.detach().cpu().numpy().copy() for v in tv}


def test_recompile_and_unfreeze_do_not_reuse_stale_gradient_slices(cuda):
    """compile(new optimizer) between training blocks (Boosted_DETR_COCO.ipynb cells 26/30) and a freeze -> train ->
    unfreeze cycle leave some variables with a slice of a retired flat gradient buffer that still holds an earlier
    step's gradients; the in-place sinks (split-K atomics accumulate!) must not write there.  The first step after
    either event has to produce the gradients a freshly built model produces for the same weights and batch."""
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg, batch = small_batch()
    _, batch2 = small_batch(seed=21)
    params = O.make_params(cfg, seed=1)

    def fresh():
        m = small_model()
        m.compile(optimizer=SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1))
        m.forward_backward(batch)
        m.set_weights_dict(params)
        return m

    def same(a, b):
        assert a.keys() == b.keys()
        for k in a:
            scale = np.abs(b[k]).max() + 1e-30
            assert np.abs(a[k] - b[k]).max() <= 1e-5 * scale, k      # split-K atomics: order-dependent last bits only

    want = _grads_after_one_step(fresh(), batch)

    # (1) train a step on another batch (the flat buffer now holds ITS gradients), recompile, first step
    m = fresh()
    m.train_step(batch2)
    m.set_weights_dict(params)
    old_flat = m.optimizer.flat_grad
    m.compile(optimizer=SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1))
    assert all(v.grad_buf is None for v in m.variables)
    same(_grads_after_one_step(m, batch), want)
    assert m.optimizer.flat_grad is not old_flat

    # (2) freeze the backbone, train, unfreeze: the backbone's slices belong to the pre-freeze buffer
    m = fresh()
    m.train_step(batch2)
    m.EncoderBackbone.trainable = False
    m.train_step(batch2)
    frozen_names = {v.name for v in m.EncoderBackbone.variables}
    assert all(v.grad_buf is None for v in m.variables if v.name in frozen_names)
    m.EncoderBackbone.trainable = True
    m.set_weights_dict(params)
    for v in m.variables:                                    # moving statistics moved during the extra steps
        if not v.trainable:
            v.assign(params[v.name])
    same(_grads_after_one_step(m, batch), want)


def test_range_guard_redoes_an_overflowing_step_on_the_fp32_forward(cuda):
    """A training-mode activation beyond 65504 (here: a BatchNorm beta of 1e5 inside the backbone) is finite in the
    reference's fp32 arithmetic but outside the f16 pairs of the 'split' forward.  The step must not emit NaN or
    touch the weights / moving statistics with garbage: the producers raise the range guard, the optimizer applies
    nothing, and train_step redoes the batch on the exact-fp32 forward - giving what a 'mixed' step gives."""
    from boosted_detr_amd import kernels as k
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg, batch = small_batch()
    params = O.make_params(cfg, seed=1)
    name = "EncoderBackbone/resnet50/conv2_block1_1_bn/beta"
    params[name] = np.full_like(params[name], 1e5)

    def fresh(policy):
        m = small_model()
        m.compile(optimizer=SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1))
        m.train_gemm_precision = "mixed"
        m.forward_backward(batch)                       # build (on the range-safe policy)
        m.set_weights_dict(params)
        m.train_gemm_precision = policy
        m.guard.resolve_at_once = True                  # resolve the step's flag snapshot at once (what fit() does)
        return m

    k.read_and_clear_overflow()
    ref = fresh("mixed")
    want = ref.logs_to_host(ref.train_step(batch))
    assert ref.range_redos == 0 and np.isfinite(want["loss"])
    m = fresh("split")
    got = m.logs_to_host(m.train_step(batch))
    assert m.range_redos == 1 and not k.read_and_clear_overflow()
    assert np.isfinite(got["loss"]) and abs(got["loss"] - want["loss"]) <= 1e-4 * abs(want["loss"])
    a, b = m.get_weights_dict(), ref.get_weights_dict()
    upstream = ("conv1_bn/moving", "conv2_block1_0_bn/moving", "conv2_block1_1_bn/moving")
    for key in a:
        assert np.isfinite(a[key]).all(), key
        if any(u in key for u in upstream):
            continue        # BatchNorms in front of the overflow saw this batch's (valid) statistic in both attempts: two EMA updates
        scale = np.abs(b[key]).max() + 1e-12
        assert np.abs(a[key] - b[key]).max() <= 1e-4 * scale, key      # weights and downstream moving statistics: one update, from the redo
    assert m.optimizer.iterations == 1 and m.steps_done == 1           # the guarded attempt applied nothing and is not counted

    # The same outside fit(): the host looks at a step's snapshot GUARD_LAG steps later, without synchronising.  Every batch
    # since the flag rose ran without an update; all of them are redone and the counters are rolled back - three overflowing
    # steps end exactly where three 'mixed' steps end (no batch lost, the learning-rate schedule not ahead).
    ref3, lag = fresh("mixed"), fresh("split")
    lag.guard.resolve_at_once = False
    for _ in range(3):
        w3 = ref3.logs_to_host(ref3.train_step(batch))
        g3 = lag.train_step(batch)
    assert lag.range_redos == 1 and lag.range_skipped == 3 and lag.GUARD_LAG == 2
    assert lag.optimizer.iterations == 3 and lag.steps_done == 3 and not k.read_and_clear_overflow()
    g3 = lag.logs_to_host(g3)
    # (three steps of a 2-image toy with batch statistics over a handful of samples: float-atomics noise and the extra EMA updates
    # of the BatchNorms upstream of the overflow already move the loss by ~1e-3 - measured 73.049 vs 72.962)
    assert abs(g3["loss"] - w3["loss"]) <= 1e-2 * abs(w3["loss"]), (g3, w3)
    a, b = lag.get_weights_dict(), ref3.get_weights_dict()
    for key in a:
        if not any(u in key for u in upstream) and "moving" not in key and np.abs(b[key]).max() > 1e-3:
            assert np.abs(a[key] - b[key]).max() <= 2e-2 * np.abs(b[key]).max(), key
    assert lag.guard_flush() is None and lag.range_redos == 1         # nothing left in flight is raised


def test_a_stale_overflow_flag_does_not_freeze_moving_statistics_under_another_policy(cuda):
    """The flag is process-global.  Left up by a guarded step that nobody polled (or by a stray pack of a tool), it must not stop
    the BatchNorm moving statistics of later 'mixed' / 'fp32' steps, which never read or clear it."""
    from boosted_detr_amd import kernels as k
    from boosted_detr_amd.training import SGD
    cfg, batch = small_batch()
    m = small_model()
    m.compile(optimizer=SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1))
    m.train_gemm_precision = "mixed"
    m.train_step(batch)
    k.overflow_flag().fill_(1)                                   # as an unpolled overflow would leave it
    name = "EncoderBackbone/resnet50/conv3_block1_1_bn/moving_mean"
    before = m.get_weights_dict()[name].copy()
    m.train_step(batch)
    after = m.get_weights_dict()[name]
    assert np.abs(after - before).max() > 0, "moving statistics stopped updating"
    k.read_and_clear_overflow()


def test_freeze_after_capture_does_not_replay_the_old_graph(cuda):
    """A captured step bakes in the trainable set, the optimizer's buffers, dropout rates and loss weights: changing any of
    them must lead to a fresh capture, never to a replay that keeps training a frozen layer (Model._graph_env)."""
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD
    cfg, host = small_batch()
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
             "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    m = small_model()
    m.compile(optimizer=SGD(1e-2, momentum=0.9, nesterov=True, clipnorm=0.1))
    m.use_graph = True
    for _ in range(4):
        m.train_step(batch)
    assert len(m._graphs) == 1
    m.EncoderBackbone.trainable = False
    w0 = {v.name: v.value.clone() for v in m.EncoderBackbone.variables if v.trainable}
    h0 = m.CategoryPredictionHead.DenseOut.kernel.value.clone()
    for _ in range(4):
        m.train_step(batch)
    torch.cuda.synchronize()
    assert len(m._graphs) == 2                                         # a second capture for the new trainable set
    for v in m.EncoderBackbone.variables:
        if v.name in w0:
            assert torch.equal(v.value, w0[v.name]), v.name            # frozen weights did not move
    assert not torch.equal(m.CategoryPredictionHead.DenseOut.kernel.value, h0)      # the rest keeps training
    m.compile(optimizer=SGD(1e-2, momentum=0.9, nesterov=True, clipnorm=0.1))
    assert not m._graphs                                               # a new optimizer retires every captured step
    for _ in range(3):
        logs = m.logs_to_host(m.train_step(batch))
    assert np.isfinite(logs["loss"])


def test_momentum_survives_a_freeze_unfreeze_cycle(cuda):
    """SGD.build after the trainable set changed keeps the velocity of every variable that stays trainable (Keras slot
    variables live per weight; Boosted_DETR_COCO.ipynb cell 30 freezes and unfreezes layers between fits)."""
    from boosted_detr_amd.training import SGD
    cfg, batch = small_batch()
    m = small_model()
    m.compile(optimizer=SGD(1e-2, momentum=0.9, nesterov=True, clipnorm=0.1))
    for _ in range(2):
        m.train_step(batch)
    v = m.CategoryPredictionHead.DenseOut.kernel
    i = [id(x) for x in m.optimizer.vars].index(id(v))
    mom = m.optimizer.mom_views[i].clone()
    assert float(mom.abs().max()) > 0
    fz = next(x for x in m.optimizer.vars if x.name.startswith(m.EncoderBackbone.scope))          # a backbone weight that is about to be frozen
    m.EncoderBackbone.trainable = False
    m.forward_backward(batch)                                          # rebuilds the flat buffers for the smaller set
    j = [id(x) for x in m.optimizer.vars].index(id(v))
    assert len(m.optimizer.vars) < 200 and torch.equal(m.optimizer.mom_views[j], mom)
    # ... and of a variable that was frozen and comes back (Keras keeps its slot variable across the freeze)
    assert fz._momentum is not None and float(fz._momentum.abs().max()) > 0
    parked = fz._momentum.clone()
    m.EncoderBackbone.trainable = True
    m.forward_backward(batch)
    k = [id(x) for x in m.optimizer.vars].index(id(fz))
    assert torch.equal(m.optimizer.mom_views[k], parked) and fz._momentum is None


@pytest.fixture
def deterministic():
    """BDETR_DETERMINISTIC mode for one test: split-K slices go through slabs + a fixed-order fold, column sums take the two-level
    reduction (kernels.set_deterministic) - two runs of one step give bit-identical weights."""
    from boosted_detr_amd import kernels as K
    prev = K.set_deterministic(True)
    yield
    K.set_deterministic(prev)


def _same_weights(a: dict, b: dict):
    bad = [k for k in a if not np.array_equal(a[k], b[k])]
    return bad


def test_graph_replayed_steps_equal_eager_steps(cuda, deterministic):
    """Model.use_graph: the third step on an input signature is captured as a chain of hipGraphs and later steps replay it.  With
    dropout on (masks keyed by a per-step seed kept in HBM) and a cosine learning-rate schedule (rate staged in HBM per
    step), six replayed steps must EQUAL six eagerly enqueued ones: in deterministic mode (no float atomics) every loss and every
    weight is the same to the last bit - a stale dropout seed, learning rate or input in a replayed graph cannot hide in a
    tolerance (round 3 compared to 20 % because of the atomics)."""
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD, CosineDecayRestarts
    from oracle import detr_oracle as O
    cfg, host = small_batch()
    params = O.make_params(cfg, seed=1)
    dev_batch = lambda b: {"image": to_device(b["image"]), "category": to_device(b["category"], torch.int32),
                           "attribute": to_device(b["attribute"], torch.int32), "bbox": to_device(b["bbox"]),
                           "num_objects": to_device(b["num_objects"], torch.int32)}
    batches = [dev_batch(host), dev_batch(small_batch(seed=21)[1])]
    runs = {}
    from boosted_detr_amd import engine
    keep_census, engine.SegmentedCapture.CENSUS = engine.SegmentedCapture.CENSUS, True         # (restored below)
    for graph in (False, True, "again"):
        m = small_model(dropout=0.1)
        m.compile(optimizer=SGD(CosineDecayRestarts(1e-3, 10, m_mul=.95, alpha=.1), momentum=.9, nesterov=True, clipnorm=.1))
        m.forward_backward(batches[0])
        m.set_weights_dict(params)
        m.use_graph = graph is True
        losses = [m.logs_to_host(m.train_step(batches[i % 2]))["loss"] for i in range(8)]
        assert (len(m._graphs) == 1) == (graph is True) and m.steps_done == 8 and m.optimizer.iterations == 8
        runs[graph] = (losses, m.get_weights_dict())
        if graph is True:
            # "kernel nodes only": no memset / memcpy node entered the captured step (a hipMemset node replayed wrongly in round 4);
            # SegmentedCapture.census() already raised inside the capture otherwise - here the count is shown to be a real one
            census = m._graph_census
            assert census.get(0, 0) > 200 and not set(census) - set(engine.SegmentedCapture.ALLOWED_NODE_TYPES), census
            print("graph node census {hipGraphNodeType: count}:", census)
    engine.SegmentedCapture.CENSUS = keep_census
    le, lg, le2 = runs[False][0], runs[True][0], runs["again"][0]
    assert all(np.isfinite(lg))
    assert le == le2 and not _same_weights(runs[False][1], runs["again"][1])           # the mode itself: two eager runs are identical
    assert le == lg, (le, lg)                                                          # every loss, bit for bit
    assert not _same_weights(runs[False][1], runs[True][1]), _same_weights(runs[False][1], runs[True][1])[:5]
    assert lg[2] != lg[4]                                                              # fresh masks / inputs per replay, not a frozen step


def test_unsynchronised_graph_replays_equal_eager_steps(cuda, deterministic):
    """Back-to-back replays with NO host read in between (the way bench.py and a training loop without per-step logging run):
    on ROCm 7.2 the second replay of a graph without a stream synchronisation in between handed NaN gradients to the optimizer
    unless the runtime's pre-built-packet path is off (boosted_detr_amd.enable_graph_replay; Model refuses graphs when that came
    too late).  Twelve unsynchronised replayed steps must leave exactly the weights of twelve eager steps (deterministic mode:
    bit for bit), no guard redo."""
    import boosted_detr_amd
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    assert boosted_detr_amd.graph_replay_is_safe(), "the test session initialised HIP before boosted_detr_amd.enable_graph_replay()"
    cfg, host = small_batch()
    params = O.make_params(cfg, seed=1)
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32),
             "attribute": to_device(host["attribute"], torch.int32), "bbox": to_device(host["bbox"]),
             "num_objects": to_device(host["num_objects"], torch.int32)}
    final = {}
    for graph in (False, True):
        m = small_model()
        m.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
        m.forward_backward(batch)
        m.set_weights_dict(params)
        m.use_graph = graph
        first = None
        for i in range(12):
            logs = m.train_step(batch)                 # no host read, no synchronisation between steps
            if i == 0:
                first = [t.clone() for t in logs["loss"]]
        m.guard_flush()
        torch.cuda.synchronize()
        assert (len(m._graphs) == 1) == graph
        assert m.range_redos == 0 and int(K.overflow_flag().item()) == 0, (graph, m.range_redos)
        assert all(bool(torch.isfinite(v.value).all()) for v in m.variables), graph
        final[graph] = (m.logs_to_host({"loss": first})["loss"], m.logs_to_host(logs)["loss"], m.get_weights_dict())
    assert final[True][0] == final[False][0] and final[True][1] == final[False][1], (final[True][:2], final[False][:2])
    assert not _same_weights(final[False][2], final[True][2]), _same_weights(final[False][2], final[True][2])[:5]
    assert final[False][1] < 0.8 * final[False][0]                                                # and it trained


def test_non_finite_gradient_raises_the_guard_and_applies_nothing(cuda):
    """A NaN born in the backward pass leaves the loss finite, so the guard's loss check cannot see it: the optimizer's norm pass
    raises the flag instead and NO tensor is updated (not even those whose own gradient is clean)."""
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD
    cfg, batch = small_batch()
    model = small_model()
    opt = SGD(learning_rate=0.05, momentum=0.9, nesterov=True, clipnorm=0.1)
    model.compile(optimizer=opt)
    model.forward_backward(batch)                      # build
    model.forward_backward(batch)
    tv = model.trainable_variables
    opt.stage_gradients(tv)
    before = [v.value.detach().clone() for v in tv]
    opt.flat_grad[opt.flat_grad.numel() // 2] = float("nan")
    flag = K.overflow_flag()
    flag.zero_()
    opt.apply_gradients(skip_flag=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1
    assert all(torch.equal(a, v.value) for a, v in zip(before, tv))
    flag.zero_()
    opt.flat_grad[opt.flat_grad.numel() // 2] = 0.0
    opt.apply_gradients(skip_flag=flag)                # a clean gradient goes through
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and any(not torch.equal(a, v.value) for a, v in zip(before, tv))


def test_a_step_that_fails_during_capture_leaves_the_stream_usable(cuda):
    """An exception inside the captured step must end the open capture (engine.SegmentedCapture.abort): the next step - eager or a fresh
    capture - runs, counters are where they were."""
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD
    cfg, host = small_batch()
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32),
             "attribute": to_device(host["attribute"], torch.int32), "bbox": to_device(host["bbox"]),
             "num_objects": to_device(host["num_objects"], torch.int32)}
    m = small_model()
    opt = SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1)
    m.compile(optimizer=opt)
    m.use_graph = True
    m.train_step(batch); m.train_step(batch)                       # two eager steps; the third captures
    real = opt.apply_gradients

    def boom(*a, **k):
        raise RuntimeError("boom")
    opt.apply_gradients = boom
    steps = (m.steps_done, opt.iterations)
    with pytest.raises(RuntimeError, match="boom"):
        m.train_step(batch)
    opt.apply_gradients = real
    assert (m.steps_done, opt.iterations) == steps and not m._graphs
    assert not torch.cuda.is_current_stream_capturing()
    loss = m.logs_to_host(m.train_step(batch))["loss"]             # captures now (or runs eagerly): either way a valid step
    assert np.isfinite(loss) and m.steps_done == steps[0] + 1


def test_replayed_step_is_bit_identical_with_the_runtime_packet_path_on(cuda):
    """The round-3 replay defect, pinned: with the ROCm 7.2 runtime's pre-built packet path ON (DEBUG_CLR_GRAPH_PACKET_CAPTURE=1, the
    runtime default) a hipMemset node inside the relaunched chain went wrong (first differing tensor: the one ops.tile_batch zero-fills)
    and NaN followed.  The library's zero fills are kernels now; this runs tools/graph_segment_checksums.py at configs[1] size in a
    process of its own (the switch is read when HIP initialises) and requires every layer output, every activation gradient crossing a
    segment cut and the gradient buffer behind every segment to be bit-identical between the eager and the replayed run, 8 synchronised
    + 10 unsynchronised steps, no non-finite entry, no guard flag."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DEBUG_CLR_GRAPH_PACKET_CAPTURE="1", SYNC_STEPS="8", STEPS="10", BDETR_DETERMINISTIC="1", BDETR_SIDE_STREAM="0", BDETR_GRAPH_SIDE="0")
    env.pop("BDETR_ZERO_MEMSET", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_segment_checksums.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = next(l for l in r.stdout.splitlines() if l.startswith("GRAPH_SEGMENT_CHECKSUMS "))
    out = json.loads(line.split(" ", 1)[1])
    assert out["weights_finite"] == {"eager": True, "graph": True}
    for kind in ("L", "F", "A", "S"):
        assert out[kind]["n"][0] == out[kind]["n"][1] > 0, (kind, out[kind])
        assert out[kind]["first_difference"] is None and out[kind]["first_nonfinite_or_flag_in_graph_run"] is None, (kind, out[kind])


@pytest.mark.parametrize("grad_policy", ["fp32", "bf16x6"])
def test_gradient_policy_of_its_own_runs_the_backward_under_it(cuda, deterministic, grad_policy):
    """Model.train_grad_precision = 'bf16x6' (three bf16 terms, six products on the 16-bit MFMA) or 'fp32' after the 'split' forward
    (bench.py's value_fp32_grade legs: no product of the step below 2^-22): the gradients ARE the ones replay_backward(policy)
    computes from the same saved forward - bit for bit in deterministic mode - and differ from the all-'split' step's; a captured
    step under that policy equals the eager one."""
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg, host = small_batch()
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
             "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    m = small_model(dropout=0.1)
    m.compile(optimizer=SGD(1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    m.forward_backward(batch)
    m.set_weights_dict(O.make_params(cfg, seed=1))
    grads = lambda: {v.name: v.grad.detach().cpu().numpy().copy() for v in m.trainable_variables if v.grad is not None}
    m.forward_backward(batch)
    g_split = grads()
    m.train_grad_precision = grad_policy
    m.forward_backward(batch, keep_tape=True)
    g_own = grads()
    m.replay_backward(grad_policy)
    g_replay = grads()
    m._kept_tape = None
    assert set(g_own) == set(g_replay) == set(g_split) and len(g_own) > 50
    assert not [k for k in g_own if not np.array_equal(g_own[k], g_replay[k])]
    assert any(not np.array_equal(g_own[k], g_split[k]) for k in g_own)
    # the same policy through the captured step
    runs = {}
    for graph in (False, True):
        mm = small_model(dropout=0.1)
        mm.compile(optimizer=SGD(1e-3, momentum=.9, nesterov=True, clipnorm=.1))
        mm.forward_backward(batch)
        mm.set_weights_dict(O.make_params(cfg, seed=1))
        mm.train_grad_precision, mm.use_graph = grad_policy, graph
        losses = [mm.logs_to_host(mm.train_step(batch))["loss"] for _ in range(5)]
        assert (len(mm._graphs) == 1) == graph
        runs[graph] = (losses, mm.get_weights_dict())
    assert runs[False][0] == runs[True][0] and not _same_weights(runs[False][1], runs[True][1])


@pytest.mark.parametrize("kind", ["detr", "boosted"])
def test_eager_steps_do_not_leak_device_memory(cuda, kind):
    """Round 5 regression: a handle that referenced itself through a VIEW stored in its own __dict__ (the stem's pooled tensor aliasing
    its f16 pair copy) is a cycle the cyclic GC cannot see - a view's `_base` edge lives in C++ - and leaked one pooled tensor per eagerly
    enqueued step (100 MB at the bench's batch; the 2,000-step soak found it: profiles/r05_soak_2000steps_eager_leak.txt).  After a
    collection, device memory held after 12 steps equals device memory held after 6."""
    import gc
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD
    cfg, host = small_batch()
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
             "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    if kind == "boosted":
        from boosted_detr_amd import parameters
        from boosted_detr_amd.boosted_model import BoostedDETR
        m = BoostedDETR(num_object_preds=10, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=2,
                        num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32, vocab_dict=parameters.synthetic_vocab(10, 4), attribute_weight=1.0)
    else:
        m = small_model()
    m.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    held = []
    for _ in range(2):
        for _ in range(6):
            m.train_step(batch)
        m.guard_flush()
        torch.cuda.synchronize()
        gc.collect()
        held.append(torch.cuda.memory_allocated())
    assert held[1] <= held[0] + (1 << 17), f"device memory grew by {(held[1] - held[0]) / 2 ** 20:.1f} MiB over six eager steps"


def test_compact_stride2_gradients_and_their_fallbacks_give_the_same_step(cuda, deterministic):
    """The gradient of a stage's last unit as a compact even-pixel tensor (ops.COMPACT_S2, round 5) against the zero-filled scatter form
    it replaces, and against the fallback in which its consumer cannot take it compact and engine.materialise expands it
    (ops.LAZY_SKIP off): every parameter gradient of a training step agrees (deterministic mode: the only difference is where zeros
    are added, so the compact / scatter pair is bit-identical)."""
    from boosted_detr_amd import ops
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg, host = small_batch()
    params = O.make_params(cfg, seed=1)
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
             "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    keep = (ops.COMPACT_S2, ops.LAZY_SKIP)
    grads = {}
    try:
        for name, (compact, lazy) in {"compact": (True, True), "scatter": (False, True), "expanded": (True, False)}.items():
            ops.COMPACT_S2, ops.LAZY_SKIP = compact, lazy
            m = small_model()
            m.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
            m.forward_backward(batch)
            m.set_weights_dict(params)
            m.forward_backward(batch)
            torch.cuda.synchronize()
            grads[name] = {v.name: v.grad.detach().clone() for v in m.trainable_variables if v.grad is not None}
    finally:
        ops.COMPACT_S2, ops.LAZY_SKIP = keep
    assert len(grads["compact"]) > 100
    bad = [k for k, g in grads["compact"].items() if not torch.equal(g, grads["scatter"][k])]
    assert not bad, bad[:5]
    for k, g in grads["compact"].items():
        e = grads["expanded"][k]
        scale = float(g.abs().max()) + 1e-30
        assert float((g - e).abs().max()) <= 1e-4 * scale, (k, float((g - e).abs().max()) / scale)      # (another order of fp32 adds and bf16-pair roundings along the skip path)


def test_side_stream_is_placed_by_measurement(cuda):
    """engine.side_stream(): a low-priority candidate is measured against the critical path's stream (how long 200 one-workgroup kernels
    take there while the candidate streams 120 passes over 64 MB, against the same ticks with no load) and kept only when it is good; a bad
    one is followed by the next, up to four.  On MI355X / ROCm 7.2 one of the four hardware queues costs the training step 80 % (DESIGN
    5c) - it shows up here as 9 x the unloaded time against 1.5 x."""
    from boosted_detr_amd import engine
    s = engine.side_stream()
    pl = engine.side_stream_placement()
    if pl is None:
        pytest.skip("side stream created without candidates (BDETR_SIDE_CANDIDATES=1 or BDETR_SIDE_PRIORITY != low)")
    assert 1 <= len(pl["tick_ms"]) <= 4 and all(t > 0 for t in pl["tick_ms"]) and pl["unloaded_ms"] > 0, pl
    assert pl["picked"] in pl["good"] and pl["tick_ms"][pl["picked"]] < engine.SIDE_BAD_RATIO * pl["unloaded_ms"], pl
    assert all(t >= engine.SIDE_BAD_RATIO * pl["unloaded_ms"] for t in pl["tick_ms"][:pl["picked"]]), pl          # whatever was skipped was bad
    assert s is engine._SIDE["candidates"][pl["picked"]] and sum(c is not None for c in engine._SIDE["candidates"]) == 1     # the others are gone
    print("side-stream candidates, ms of the critical path's ticks under each:", pl["tick_ms"], "unloaded", pl["unloaded_ms"], "picked", pl["picked"])
