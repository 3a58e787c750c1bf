"""Auxiliary decoder losses on the GPU (DETR(use_intermediate_losses=True)): the grouped-row BatchNorm kernels and the tiled matcher
entry points against fp64 torch / the plain entry points, the model against the CPU reference tests/_aux_ref.py (3 decoder blocks, stacked
and looped), and the option's effect on everything around it (option off, graph capture, panoptic head, checkpoints, BoostedDETR).

Seed of the parity batch: 1234 - checked on the CPU that the fp32 and the fp64 reference give the same assignment at every decoder block
for it (block 0/1/2 assign image 1's objects to queries [41,0,2,15,43,18,5] / [41,35,49,19,33,38,12] / [10,35,8,16,4,38,6])."""
import os
import types

import numpy as np
import pytest
import torch

import _aux_ref as R
from _close import assert_logits, check_predictions
from test_kernels_gpu import close, dev, rnd
from test_model_gpu import grad_report

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-3, 0.99
SHAPES = [(1, 100, 256), (3, 100, 1024), (4, 7, 64), (2, 65, 48), (6, 1600, 1024)]     # (G, R, C)


# ---------------------------------------------------------------- kernels
def _bn_case(G, R, C):
    x = (rnd(G * R, C, seed=1) * 2 + 0.5).view(G, R, C) + 0.3 * torch.arange(G).view(G, 1, 1)       # every group its own mean
    x = (x * (1 + 0.25 * torch.arange(G).view(G, 1, 1))).reshape(G * R, C).contiguous()               # ... and variance
    return x, 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3), rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5, rnd(G * R, C, seed=6)


@pytest.mark.parametrize("G,R,C", SHAPES)
def test_grouped_batchnorm_training(cuda, G, R, C):
    from boosted_detr_amd import kernels as k
    x, gamma, beta, mm, mv, dout = _bn_case(G, R, C)
    xd, gd, bd, mmd, mvd, doutd = dev(x), dev(gamma), dev(beta), dev(mm), dev(mv), dev(dout)
    k.read_and_clear_overflow()                           # (a raised range guard would hold the moving statistics back)
    mean, rstd, var = k.bn_rows_stats(xd, G, EPS)
    out = k.bn_rows_apply(xd, G, mean, rstd, gd, bd, var, MOMENTUM, mmd, mvd)
    x64 = x.double().view(G, R, C).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m, v = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
    ref = (x64 - m) / torch.sqrt(v + EPS) * g64 + b64
    close(out.view(G, R, C), ref)
    close(mean, m.squeeze(1))
    close(rstd, 1 / torch.sqrt(v.squeeze(1) + EPS))
    close(var, v.squeeze(1))
    mm_ref, mv_ref = mm.double(), mv.double()
    for g in range(G):                                    # G sequential keras calls: one update per group, in group order
        mm_ref = mm_ref * MOMENTUM + m[g, 0].detach() * (1 - MOMENTUM)
        mv_ref = mv_ref * MOMENTUM + v[g, 0].detach() * (1 - MOMENTUM)
    close(mmd, mm_ref)
    close(mvd, mv_ref)
    ref.backward(dout.double().view(G, R, C))
    first = k.bn_rows_bwd(doutd, xd, G, mean, rstd, gd, False)
    again = k.bn_rows_bwd(doutd, xd, G, mean, rstd, gd, False)
    for a, b in zip(first, again):
        assert torch.equal(a, b)                          # no float atomics: bit-reproducible
    dx, dgamma, dbeta = first
    close(dx.view(G, R, C), x64.grad)
    close(dgamma, g64.grad)
    close(dbeta, b64.grad)


@pytest.mark.parametrize("G,R,C", SHAPES)
def test_grouped_batchnorm_frozen(cuda, G, R, C):
    from boosted_detr_amd import kernels as k
    x, gamma, beta, mm, mv, dout = _bn_case(G, R, C)
    xd, gd, bd, mmd, mvd, doutd = dev(x), dev(gamma), dev(beta), dev(mm), dev(mv), dev(dout)
    mean, rstd = k.bn_stats_frozen(mmd, mvd, EPS)
    out = k.bn_rows_apply(xd, G, mean, rstd, gd, bd)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = (x64 - mm.double()) / torch.sqrt(mv.double() + EPS) * g64 + b64
    close(out, ref)
    assert torch.equal(mmd.cpu(), mm) and torch.equal(mvd.cpu(), mv)           # moving statistics untouched
    ref.backward(dout.double())
    first = k.bn_rows_bwd(doutd, xd, G, mean, rstd, gd, True)
    again = k.bn_rows_bwd(doutd, xd, G, mean, rstd, gd, True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    close(first[0], x64.grad)
    close(first[1], g64.grad)
    close(first[2], b64.grad)


@pytest.mark.parametrize("G,R,C", [s for s in SHAPES if s[0] > 1])
def test_grouped_batchnorm_groups_do_not_leak(cuda, G, R, C):
    """A group's statistics, output and input gradient are bit-identical when another group's rows change."""
    from boosted_detr_amd import kernels as k
    x, gamma, beta, mm, mv, dout = _bn_case(G, R, C)
    x2 = x.clone().view(G, R, C)
    x2[G - 1] = x2[G - 1] * 3.0 - 7.0
    gd, bd, doutd = dev(gamma), dev(beta), dev(dout)
    res = []
    for xx in (x, x2.reshape(G * R, C)):
        xd = dev(xx)
        mean, rstd, var = k.bn_rows_stats(xd, G, EPS)
        out = k.bn_rows_apply(xd, G, mean, rstd, gd, bd)
        dx, _, _ = k.bn_rows_bwd(doutd, xd, G, mean, rstd, gd, False)
        res.append((mean, rstd, var, out.view(G, R, C), dx.view(G, R, C)))
    for a, b in zip(*res):
        assert torch.equal(a[:G - 1], b[:G - 1])
        assert not torch.equal(a[G - 1], b[G - 1])


def test_grouped_batchnorm_guard_keeps_moving_statistics(cuda):
    """Non-finite batch statistics raise the range guard, and the moving statistics are then left alone (bdetr_bn_stats' convention)."""
    from boosted_detr_amd import kernels as k
    x, gamma, beta, mm, mv, _ = _bn_case(2, 7, 64)
    x[9, 5] = float("inf")
    mmd, mvd = dev(mm), dev(mv)
    k.read_and_clear_overflow()
    xd = dev(x)
    mean, rstd, var = k.bn_rows_stats(xd, 2, EPS)
    k.bn_rows_apply(xd, 2, mean, rstd, dev(gamma), dev(beta), var, MOMENTUM, mmd, mvd)
    assert k.read_and_clear_overflow()
    assert torch.equal(mmd.cpu(), mm) and torch.equal(mvd.cpu(), mv)


def test_tiled_matcher_equals_per_block_calls(cuda):
    """bdetr_{cost_matrix,lsa,set_loss}_tiled over L stacked prediction blocks == the plain entry points called per block, bit for bit
    (match, cost, all six loss rows, the three gradients)."""
    from boosted_detr_amd import kernels as k
    L, B, M, N, C, A = 3, 2, 6, 11, 9, 5
    g = torch.Generator().manual_seed(3)
    cat = torch.softmax(torch.randn(L * B, N, C, generator=g), -1)
    att, box = torch.sigmoid(torch.randn(L * B, N, A, generator=g)), torch.rand(L * B, N, 4, generator=g) * 0.8
    ids = torch.randint(2, C, (B, M), generator=g).int()
    hot = (torch.rand(B, M, A, generator=g) > 0.6).float()
    bbox, nobj = torch.rand(B, M, 4, generator=g) * 0.5 + 0.05, torch.tensor([4, 6], dtype=torch.int32)
    catd, attd, boxd, idsd, hotd, bboxd, nobjd = dev(cat), dev(att), dev(box), dev(ids, torch.int32), dev(hot), dev(bbox), dev(nobj, torch.int32)
    d = k.loss_desc(L * B, M, N, C, A, 1000.0, 100.0, 1.0, 100.0)
    cost = k.cost_matrix(d, catd, attd, boxd, idsd, hotd, bboxd, nobjd, period=B)
    match = k.lsa(cost, nobjd, period=B)
    losses, dc, da, db = k.set_loss(d, catd, attd, boxd, idsd, hotd, bboxd, nobjd, match, loss_scale=0.5, period=B)
    d1 = k.loss_desc(B, M, N, C, A, 1000.0, 100.0, 1.0, 100.0)
    for l in range(L):
        s = slice(l * B, (l + 1) * B)
        c1 = k.cost_matrix(d1, catd[s], attd[s], boxd[s], idsd, hotd, bboxd, nobjd)
        m1 = k.lsa(c1, nobjd)
        l1, dc1, da1, db1 = k.set_loss(d1, catd[s], attd[s], boxd[s], idsd, hotd, bboxd, nobjd, m1, loss_scale=0.5)
        assert torch.equal(cost[s], c1) and torch.equal(match[s], m1) and torch.equal(losses[:, s], l1)
        assert torch.equal(dc[s], dc1) and torch.equal(da[s], da1) and torch.equal(db[s], db1)
    assert int((match >= 0).sum()) == L * 10


# ---------------------------------------------------------------- model parity against tests/_aux_ref.py
def _detr(cfg, **kw):
    from boosted_detr_amd import parameters, transformers
    from boosted_detr_amd.model import DETR
    transformers.AttentionBlock.dropout_rate = transformers.FeedForwardBlock.dropout_rate = 0.0
    vocab = parameters.synthetic_vocab(cfg.num_categories - 2, cfg.num_attributes - 2)
    return DETR(num_object_preds=cfg.num_object_preds, image_size=cfg.image_size, num_encoder_blocks=cfg.num_encoder_blocks,
                num_encoder_heads=cfg.num_encoder_heads, encoder_dim=cfg.encoder_dim, num_decoder_blocks=cfg.num_decoder_blocks,
                num_decoder_heads=cfg.num_decoder_heads, decoder_dim=cfg.decoder_dim, num_panoptic_heads=1, panoptic_dim=32,
                vocab_dict=vocab, attribute_weight=cfg.attribute_weight, pad_value="<PAD>", oov_value="<OOV>", **kw)


def _with_env(name, value, fn):
    keep = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if keep is None:
            del os.environ[name]
        else:
            os.environ[name] = keep


@pytest.fixture(scope="module")
def reference(cuda):
    from oracle import detr_oracle as O
    cfg = R.SMALL_CFG
    batch = O.make_batch(cfg, seed=1234, **R.SMALL_BATCH_ARGS)
    params = O.make_params(cfg, seed=0)
    out32, g32 = R.train_step_grads(cfg, params, batch, dtype=torch.float32)
    out64, g64 = R.train_step_grads(cfg, params, batch, dtype=torch.float64)
    L, (B, M) = cfg.num_decoder_blocks, batch["category"].shape
    for l in range(L):
        assert np.array_equal(out32.matches(l, B, M), out64.matches(l, B, M)), "fp32 and fp64 references disagree on an assignment: take another seed"
    return types.SimpleNamespace(cfg=cfg, batch=batch, params=params, out32=out32, g32=g32, out64=out64, g64=g64, L=L, B=B, M=M)


@pytest.fixture(scope="module")
def steps(reference):
    """One parity step per setting of BDETR_AUX_STACKED: {setting: snapshot of everything the tests below compare}."""
    ref, snaps = reference, {}
    for setting in ("1", "0"):
        model = _with_env("BDETR_AUX_STACKED", setting, lambda: _detr(ref.cfg, use_intermediate_losses=True))
        assert model.aux_stacked == (setting == "1") and model.use_intermediate_losses is True
        model.forward_backward(ref.batch)             # build-by-first-call, then the reference's weights
        model.set_weights_dict(ref.params)
        y_pred = model.forward_backward(ref.batch)
        torch.cuda.synchronize()
        heads = (model.CategoryPredictionHead, model.AttributePredictionHead, model.BoxPredictionHead)
        snaps[setting] = types.SimpleNamespace(
            model=model, y_pred=[t.clone() for t in y_pred], preds=[[t.clone() for t in p] for p in model.aux_predictions],
            logits=[[t.clone() for t in p] for p in model.aux_logits], last_logits=[h.last_logits.clone() for h in heads],
            matches=model.aux_matches.cpu().numpy(), last_match=model.loss_fn.last_match.cpu().numpy(), last_cost=model.loss_fn.last_cost.clone(),
            logs=model.logs_to_host(model.step_logs()), moving=model.get_weights_dict(),
            grads={v.name: v.grad_numpy().astype(np.float64) for v in model.trainable_variables})
    return snaps


@pytest.mark.parametrize("setting", ["1", "0"])
def test_per_layer_predictions_logits_and_matches(reference, steps, setting):
    ref, s = reference, steps[setting]
    assert len(s.preds) == ref.L and s.matches.shape == (ref.L, ref.B, ref.M) and s.matches.dtype == np.int32
    for l in range(ref.L):
        heads = [types.SimpleNamespace(last_logits=t) for t in s.logits[l]]
        rep = check_predictions(heads, s.preds[l], ref.out64.layers[l])
        print(setting, l, {k: f"{v['max_abs_err']:.2e}" for k, v in rep.items()})
        assert np.array_equal(s.matches[l], ref.out64.matches(l, ref.B, ref.M)), l           # bit-exact
        assert np.array_equal(s.preds[l][0].cpu().numpy().argmax(-1), ref.out32.layers[l].cat_preds.detach().numpy().argmax(-1))
    # what stays the LAST block's: the returned predictions, the heads' last_logits, loss_fn.last_match / last_cost
    for got, want in zip(s.y_pred, s.preds[-1]):
        assert torch.equal(got, want)
    for got, want in zip(s.last_logits, s.logits[-1]):
        assert torch.equal(got, want)
    assert np.array_equal(s.last_match, s.matches[-1]) and s.last_cost.shape == (ref.B, ref.M, ref.cfg.num_object_preds)
    assert not np.array_equal(s.matches[0], s.matches[-1])        # (the blocks do assign differently: "last" is a real statement)


@pytest.mark.parametrize("setting", ["1", "0"])
def test_summed_losses_and_last_layer_iou(reference, steps, setting):
    ref, logs = reference, steps[setting].logs
    want = dict(ref.out64.metrics, loss=ref.out64.loss_vector)
    assert sorted(logs) == sorted(want)
    for k, w in want.items():
        w = float(w.detach().double().mean())
        print(setting, k, logs[k], w)
        assert abs(logs[k] - w) <= 1e-3 * abs(w) + 1e-7, (k, logs[k], w)
    one = float(ref.out64.layers[-1].loss.total.detach().mean())
    assert logs["loss"] > 1.5 * one           # a sum over three blocks - the step that ignores the option logs one block's loss


@pytest.mark.parametrize("setting", ["1", "0"])
def test_heads_moving_statistics_after_one_step(reference, steps, setting):
    ref, model = reference, steps[setting].model
    model.set_weights_dict(ref.params)
    model.forward_backward(ref.batch)
    got = model.get_weights_dict()
    for name, w in ref.out64.new_moving.items():
        assert_logits(got[name], w.numpy(), name)
    for name in R.HEAD_MOVING:                # three chained updates, not one
        once = ref.params[name] * MOMENTUM + (1 - MOMENTUM) * (ref.out64.head_means if name.endswith("mean") else ref.out64.head_vars)[name.rsplit("/", 1)[0]][-1].numpy()
        assert np.abs(got[name] - once).max() > 10 * np.abs(got[name] - ref.out64.new_moving[name].numpy()).max(), name


@pytest.mark.parametrize("setting", ["1", "0"])
def test_gradients(reference, steps, setting):
    ref, model = reference, steps[setting].model
    model.set_weights_dict(ref.params)
    model.forward_backward(ref.batch)
    rows = grad_report(model, ref.g32, ref.g64)
    assert len(rows) > 100
    print("\n".join(f"{n}: gpu {a:.2e}/{b:.2e} cpu32 {c:.2e}/{d:.2e}" for a, b, c, d, n in rows[:6]))
    bad = [r for r in rows if r[1] > max(4.0 * r[3], 5e-3) or r[0] > max(4.0 * r[2], 5e-2)]
    assert not bad, "\n".join(f"{n}: gpu {a:.2e}/{b:.2e} cpu32 {c:.2e}/{d:.2e}" for a, b, c, d, n in bad[:12])


def test_stacked_against_looped(reference, steps):
    """Identical assignments at every block; loss and gradient differences are printed (both already hold the parity bars)."""
    a, b = steps["1"], steps["0"]
    assert np.array_equal(a.matches, b.matches)
    print("loss: stacked", a.logs["loss"], "looped", b.logs["loss"], "rel", abs(a.logs["loss"] - b.logs["loss"]) / abs(b.logs["loss"]))
    worst = sorted(((np.linalg.norm(a.grads[n] - g) / (np.linalg.norm(g) + 1e-300), n) for n, g in b.grads.items() if np.abs(g).max() > 0), reverse=True)
    print("gradients, relative L2 stacked vs looped, worst 5:", [(f"{e:.2e}", n) for e, n in worst[:5]])


@pytest.mark.parametrize("setting", ["1", "0"])
def test_head_parameter_sinks(cuda, monkeypatch, setting):
    """Stacked: every head parameter receives exactly ONE gradient contribution, written in place into its slice of the optimizer's flat
    gradient buffer (no temporary, no axpy); looped: one contribution per decoder block, the first of them in place."""
    from boosted_detr_amd import ops
    from boosted_detr_amd.training import SGD
    from test_training_gpu import small_batch, small_model
    monkeypatch.setenv("BDETR_AUX_STACKED", setting)
    _, batch = small_batch()
    m = small_model(use_intermediate_losses=True)
    m.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    for _ in range(2):
        m.train_step(batch)
    seen = {}
    commit = ops.GradSink.commit

    def spy(self):
        seen.setdefault(self.var.name, []).append(self.mode)
        return commit(self)

    monkeypatch.setattr(ops.GradSink, "commit", spy)
    m.forward_backward(batch)
    torch.cuda.synchronize()
    head_vars = [v for v in m.trainable_variables if "PredictionHead" in v.name]
    assert len(head_vars) == 18
    for v in head_vars:
        assert seen[v.name] == (["direct"] if setting == "1" else ["direct", "temp"]), (v.name, seen[v.name])
        assert v.grad is v.grad_buf and v.grad.data_ptr() == v.grad_buf.data_ptr()
        flat = m.optimizer.flat_grad
        assert flat.data_ptr() <= v.grad.data_ptr() < flat.data_ptr() + flat.numel() * 4


# ---------------------------------------------------------------- around the option
@pytest.fixture
def deterministic():
    from boosted_detr_amd import kernels as K
    prev = K.set_deterministic(True)
    yield
    K.set_deterministic(prev)


def _device_batch(host):
    from boosted_detr_amd.engine import to_device
    return {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
            "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}


def _run(model, params, batches, steps, toggle_at=None):
    from boosted_detr_amd.training import SGD
    model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    model.forward_backward(batches[0])
    model.set_weights_dict(params)
    losses = []
    for i in range(steps):
        if toggle_at is not None and i == toggle_at:
            model.use_intermediate_losses = not model.use_intermediate_losses
        losses.append(model.logs_to_host(model.train_step(batches[i % len(batches)]))["loss"])
    return losses, model.get_weights_dict()


def test_option_off_is_the_unchanged_step(cuda, deterministic):
    from oracle import detr_oracle as O
    from test_training_gpu import small_batch, small_model
    cfg, host = small_batch()
    params, batches = O.make_params(cfg, seed=1), [_device_batch(host)]
    plain = small_model()
    assert plain.use_intermediate_losses is False and "use_intermediate_losses" not in plain.get_config()
    off = small_model(use_intermediate_losses=False)
    on = small_model(use_intermediate_losses=True)
    assert on.get_config()["use_intermediate_losses"] is True
    la, wa = _run(plain, params, batches, 2)
    lb, wb = _run(off, params, batches, 2)
    assert la == lb and not [k for k in wa if not np.array_equal(wa[k], wb[k])]
    assert off.aux_predictions is None and off.aux_matches is None
    lc, wc = _run(on, params, batches, 2)
    assert lc[0] > 1.5 * la[0] and [k for k in wa if not np.array_equal(wa[k], wc[k])]        # ... and on is another step


def test_graph_replayed_aux_steps_equal_eager_steps(cuda, deterministic):
    """Six graph-replayed steps with the option on leave the weights of six eager ones, bit for bit (two eager warm-up steps in front
    of the capture in both runs); toggling the option afterwards is a fresh capture, never a replay of the other step."""
    from boosted_detr_amd import engine
    from oracle import detr_oracle as O
    from test_training_gpu import small_batch, small_model
    cfg, host = small_batch()
    params = O.make_params(cfg, seed=1)
    batches = [_device_batch(host), _device_batch(small_batch(seed=21)[1])]
    keep_census, engine.SegmentedCapture.CENSUS = engine.SegmentedCapture.CENSUS, True
    try:
        runs, models = {}, {}
        for graph in (False, True):
            m = models[graph] = small_model(dropout=0.1, use_intermediate_losses=True)
            m.use_graph = graph
            runs[graph] = _run(m, params, batches, 8)
            assert (len(m._graphs) == 1) == graph and m.steps_done == 8
        census = models[True]._graph_census
        assert not set(census) - set(engine.SegmentedCapture.ALLOWED_NODE_TYPES), census
        assert runs[False][0] == runs[True][0], (runs[False][0], runs[True][0])
        bad = [k for k in runs[False][1] if not np.array_equal(runs[False][1][k], runs[True][1][k])]
        assert not bad, bad[:5]
        # toggle: the next steps run eagerly under a NEW signature (two warm-up steps), then a second capture joins the first
        after = {}
        for graph in (False, True):
            m = models[graph]
            m.use_intermediate_losses = False
            losses = []
            for i in range(4):
                losses.append(m.logs_to_host(m.train_step(batches[i % 2]))["loss"])
                if graph:
                    assert len(m._graphs) == (1 if i < 2 else 2), (i, len(m._graphs))
            after[graph] = (losses, m.get_weights_dict())
        assert after[False][0] == after[True][0]
        assert not [k for k in after[False][1] if not np.array_equal(after[False][1][k], after[True][1][k])]
        assert after[True][0][0] < 0.75 * runs[True][0][-2]          # one block's loss now, not two blocks' (same batch parity)
    finally:
        engine.SegmentedCapture.CENSUS = keep_census


def test_panoptic_mask_loss_uses_the_last_layers_match(cuda):
    from boosted_detr_amd import kernels as K
    from test_panoptic_train_gpu import _small_head_batch
    from boosted_detr_amd import parameters, transformers
    from boosted_detr_amd.model import DETR
    transformers.AttentionBlock.dropout_rate = transformers.FeedForwardBlock.dropout_rate = 0.0
    model = DETR(num_object_preds=30, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=2,
                 num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32, vocab_dict=parameters.synthetic_vocab(10, 4),
                 attribute_weight=1.0, train_panoptic_head=True, use_intermediate_losses=True)
    batch = _small_head_batch()
    model.forward_backward(batch)
    seen = {}
    plain = model.MaskLoss.call

    def spy(masks_pred, masks, match, num_objects, training=False):
        seen.update(masks_pred=masks_pred, masks=masks, match=match.clone(), num_objects=num_objects)
        return plain(masks_pred, masks, match, num_objects, training=training)

    model.MaskLoss.call = spy
    model.forward_backward(batch)
    torch.cuda.synchronize()
    matches = model.aux_matches
    assert matches.shape[0] == 2 and torch.equal(seen["match"], matches[-1]) and torch.equal(model.loss_fn.last_match, matches[-1])
    want, _ = K.mask_loss(seen["masks_pred"], seen["masks"].reshape(2, -1, seen["masks_pred"].shape[-1]), matches[-1].contiguous(), seen["num_objects"],
                          model.mask_weight, model.loss_fn.loss_scale, want_grads=False)
    got = model.step_logs()["Mask_Loss"][0]
    assert torch.equal(got, want)
    if not torch.equal(matches[0], matches[-1]):          # fed the FIRST block's match the loss is another number
        other, _ = K.mask_loss(seen["masks_pred"], seen["masks"].reshape(2, -1, seen["masks_pred"].shape[-1]), matches[0].contiguous(),
                               seen["num_objects"], model.mask_weight, model.loss_fn.loss_scale, want_grads=False)
        assert not torch.equal(got, other)
    logs = model.logs_to_host(model.step_logs())
    assert len(model.step_logs()["loss"]) == 3 and np.isfinite(logs["loss"])          # two blocks' losses + the mask loss


def test_checkpoint_moves_between_option_on_and_off(cuda, tmp_path):
    from test_training_gpu import small_batch, small_model
    from boosted_detr_amd.training import SGD
    _, host = small_batch()
    batch = _device_batch(host)
    on = small_model(use_intermediate_losses=True)
    on.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    for _ in range(2):
        on.train_step(batch)
    path = str(tmp_path / "aux")
    on.save_weights(path)
    off = small_model()
    off.forward_backward(batch)
    assert sorted(v.name for v in off.variables) == sorted(v.name for v in on.variables)        # no new variables
    off.load_weights(path)
    for a, b in zip(on.predict_raw({"image": batch["image"]}), off.predict_raw({"image": batch["image"]})):
        assert torch.equal(a, b)
    on2 = small_model(use_intermediate_losses=True)
    on2.forward_backward(batch)
    off.save_weights(str(tmp_path / "plain"))
    on2.load_weights(str(tmp_path / "plain"))
    for a, b in zip(on.predict_raw({"image": batch["image"]}), on2.predict_raw({"image": batch["image"]})):
        assert torch.equal(a, b)


def test_boosted_detr_refuses_the_option(cuda):
    from boosted_detr_amd import parameters
    from boosted_detr_amd.boosted_model import BoostedDETR
    with pytest.raises(ValueError, match="use_intermediate_losses"):
        BoostedDETR(num_object_preds=10, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=2,
                    num_decoder_heads=8, decoder_dim=256, vocab_dict=parameters.synthetic_vocab(10, 4), use_intermediate_losses=True)
