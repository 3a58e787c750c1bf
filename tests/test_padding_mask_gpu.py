"""Padding masks on the GPU (include/bdetr.h K35; the batch key `valid_region`): the token-mask kernel bit for bit against the integer
rule under the guard arena, DETR and BoostedDETR with the key against the oracle with the mask (tests/_padding_mask_ref.py, bars of
tests/test_model_gpu.py), a full-image region against the call without the key, the captured step with regions that change from
step to step, Augmentations' output, the refusals, and the inference entry points."""
import numpy as np
import pytest
import torch

import _guard
import _padding_mask_ref as R
from _close import assert_elementwise, assert_logits, check_predictions
from test_model_gpu import build_model, check_grads, heads_of
from test_training_gpu import deterministic, small_batch, small_model          # noqa: F401  (deterministic is a fixture)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the kernel
def _one_row(h, r):
    top = h // r
    return top, (2 * h) // r - top           # holds the centre of token row 1 and no other


def _region_sets(B, h, w, r, c):
    top1, height1 = _one_row(h, r)
    rows = {"full": [0, 0, h, w], "model case": [16, 0, 120, 150], "none": [1, 1, 1, 1], "one row": [top1, 0, height1, w],
            "corner": [h // 2, w // 3, h - h // 2, w - w // 3]}
    names = list(rows)
    sets = [[rows[n]] * B for n in names]
    sets += [[rows[names[(k + b) % len(names)]] for b in range(B)] for k in range(len(names))]      # regions that differ per image
    return rows, [np.asarray(s, np.int32) for s in sets]


@pytest.mark.parametrize("B,h,w,r,c", [(2, 224, 224, 7, 7), (3, 200, 300, 7, 7), (2, 560, 560, 18, 18), (2, 800, 1333, 25, 42)])
def test_kernel_equals_integer_rule_under_guard(cuda, B, h, w, r, c):
    from boosted_detr_amd import kernels as K
    rows, sets = _region_sets(B, h, w, r, c)
    assert R.token_keep([rows["full"]], h, w, r, c).all() and not R.token_keep([rows["none"]], h, w, r, c).any()
    assert R.token_keep([rows["one row"]], h, w, r, c).reshape(r, c).sum(1).tolist() == [0, c] + [0] * (r - 2)
    assert 0 < R.token_keep([rows["model case"]], h, w, r, c).sum() < r * c

    def body(region):
        dev_region = _guard.ACTIVE[-1].place(region)
        mask = K.token_key_mask(dev_region, h, w, r, c)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (B, 1, 1, r * c) and mask.is_contiguous()
        got = mask.view(torch.uint8).cpu().numpy().reshape(B, r * c)
        want = R.token_keep(region, h, w, r, c)
        assert np.array_equal(got, want.astype(np.uint8)), np.argwhere(got != want)[:8]         # the bytes are 0 / 1, nothing else

    for region in sets:
        assert _guard.run_guarded(cuda, body, region) >= 1       # both fills: a byte nobody wrote differs between the runs


def test_kernel_refuses_bad_operands(cuda):
    from boosted_detr_amd import _lib, kernels as K
    from boosted_detr_amd.engine import to_device
    good = to_device(R.MODEL_REGIONS, torch.int32)
    with pytest.raises(ValueError):
        K.token_key_mask(good.reshape(4, 2), 224, 224, 7, 7)
    with pytest.raises(_lib.BdetrError):
        K.token_key_mask(good.long(), 224, 224, 7, 7)
    with pytest.raises(_lib.BdetrError):
        K.token_key_mask(good, 224, 224, 0, 7)
    with pytest.raises(_lib.BdetrError):
        K.token_key_mask(good, 224, (1 << 20) + 1, 7, 7)


# ---------------------------------------------------------------- 2. DETR against the oracle with the mask
def _with_region(batch, regions=R.MODEL_REGIONS):
    return dict(batch, valid_region=np.array(regions, np.int32))


def _run_pair(case, boosted):
    cfg, batch, params = R.model_case() if case == "model" else R.boosted_case()
    model = build_model(cfg, boosted)
    data = _with_region(batch)
    model.forward_backward(data)                 # build-by-first-call, then the oracle's weights
    model.set_weights_dict(params)
    y_pred = model.forward_backward(data)
    torch.cuda.synchronize()
    out32, g32 = R.reference(case, True, 32)
    out64, g64 = R.reference(case, True, 64)
    return cfg, batch, params, data, model, y_pred, out32, g32, out64, g64


@pytest.fixture(scope="module")
def detr_case(cuda):
    return _run_pair("model", False)


def test_detr_predictions_and_logits(detr_case):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    rep = check_predictions(heads_of(model), y_pred, out64)
    print({k: (f"{v['max_abs_err']:.2e}", f"{v['max_rel_err_above_atol']:.2e}") for k, v in rep.items()})
    assert np.array_equal(y_pred[0].cpu().numpy().argmax(-1), out32.cat_preds.detach().numpy().argmax(-1))        # class ids: bit-exact


def test_detr_match_indices_bit_exact(detr_case):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    match = model.loss_fn.last_match.cpu().numpy()
    assert np.array_equal(match, R.match_matrix(out32, *match.shape))          # (the unmasked model's differs: test_padding_mask_cpu.py)


def test_detr_logged_values(detr_case):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    logs = model.logs_to_host(model.step_logs())
    want = {"loss": out32.loss_vector, **{k: out32.metrics[k] for k in ("Category_Loss", "Attribute_Loss", "Box_Loss", "Existence_Loss", "IOU")}}
    assert len(want) == 6
    for k, w in want.items():
        w = float(w.detach().double().mean())
        print(k, logs[k], w)
        assert abs(logs[k] - w) <= 1e-3 * abs(w) + 1e-7, (k, logs[k], w)


def test_detr_gradients(detr_case):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    model.set_weights_dict(params)
    model.forward_backward(data)
    check_grads(model, cfg, params, batch, g32=g32, g64=g64)


def test_detr_moving_statistics(detr_case):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    model.set_weights_dict(params)
    model.forward_backward(data)
    got = model.get_weights_dict()
    assert len(out32.new_moving) > 100
    for name, w in out32.new_moving.items():
        assert_logits(got[name], w.numpy(), name)


def _inference_reference(cfg, batch, params):
    from oracle import detr_oracle as O
    net = R.MaskedNet(cfg, params, R.keep_of(cfg, batch, R.MODEL_REGIONS), dtype=torch.float64)
    return O.forward(net, {"image": batch["image"]}, training=False)


def test_detr_inference_raw(detr_case):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    model.set_weights_dict(params)
    inputs = {"image": batch["image"], "valid_region": data["valid_region"]}
    got = model(inputs, training=False, raw=True)
    ref = _inference_reference(cfg, batch, params)
    for name, g, w in zip(("category", "attribute", "box"), got, (ref.cat_preds, ref.attribute_preds, ref.box_preds)):
        assert_elementwise(g.cpu().numpy(), w.detach().numpy(), "inference " + name)
    assert np.array_equal(got[0].cpu().numpy().argmax(-1), ref.cat_preds.detach().numpy().argmax(-1))


# ---------------------------------------------------------------- 8. predict_raw and detections
def test_predict_raw_and_detections_take_the_key(detr_case):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    model.set_weights_dict(params)
    inputs = {"image": batch["image"], "valid_region": data["valid_region"]}
    raw = model.predict_raw(inputs)
    det = model.detections(inputs)
    assert torch.equal(det["boxes"], raw[2])
    ref = _inference_reference(cfg, batch, params)
    assert_elementwise(raw[2].cpu().numpy(), ref.box_preds.detach().numpy(), "predict_raw boxes")
    without = model.predict_raw({"image": batch["image"]})
    assert not torch.equal(without[2][1], raw[2][1])              # image 1's padding tokens were attended to without the key
    # a device tensor is the same entry
    from boosted_detr_amd.engine import to_device
    on_device = model.predict_raw({"image": batch["image"], "valid_region": to_device(data["valid_region"], torch.int32)})
    assert all(torch.equal(a, b) for a, b in zip(on_device, raw))


# ---------------------------------------------------------------- 3. BoostedDETR
def test_boosted_three_learners_with_the_key(cuda):
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = _run_pair("boosted", True)
    for name, got, want in zip(("category", "attribute", "box"), y_pred, (out64.cat_preds, out64.attribute_preds, out64.box_preds)):
        assert_elementwise(got.cpu().numpy(), want.detach().numpy(), name)
    for i in range(3):
        for head, kind in zip(heads_of(model, i), ("Category", "Attribute", "Box")):
            key = f"{kind}PredictionHead_{i}/logits"
            assert_logits(head.last_logits.cpu().numpy(), out64.probes[key].detach().numpy(), key)
    logs = model.logs_to_host(model.step_logs())
    want = float(out32.loss_vector.detach().mean())
    assert abs(logs["loss"] - want) <= 1e-3 * abs(want), (logs["loss"], want)


# ---------------------------------------------------------------- 4. a full-image region is the call without the key
def _step_bits(model, params, data):
    model.set_weights_dict(params)
    y = [t.clone() for t in model.forward_backward(data)]
    logs = model.logs_to_host(model.step_logs())
    grads = {v.name: v.grad_numpy().copy() for v in model.variables if v.trainable}
    return y, logs, grads


def test_full_image_region_equals_no_key_bit_for_bit(cuda, deterministic):
    cfg, batch, params = R.model_case()
    model = build_model(cfg)
    model.forward_backward(batch)
    h, w = batch["image"].shape[1:3]
    full = np.array([[0, 0, h, w]] * 2, np.int32)
    ya, la, ga = _step_bits(model, params, batch)
    yb, lb, gb = _step_bits(model, params, _with_region(batch, full))
    assert all(torch.equal(a, b) for a, b in zip(ya, yb))
    assert la == lb, (la, lb)
    assert len(ga) > 100 and not [k for k in ga if not np.array_equal(ga[k], gb[k])]
    yc, lc, gc = _step_bits(model, params, _with_region(batch))                 # ... and a region with padding is another step
    assert lc != la and not torch.equal(ya[0], yc[0])


# ---------------------------------------------------------------- 5. the captured step
SMALL_REGIONS = [[[0, 0, 64, 64], [0, 0, 32, 64]], [[0, 32, 64, 32], [20, 20, 40, 40]], [[0, 0, 64, 64], [32, 0, 32, 64]],
                 [[10, 0, 30, 64], [0, 0, 64, 30]], [[0, 0, 64, 64], [0, 0, 64, 64]], [[40, 40, 24, 24], [0, 0, 20, 64]],
                 [[0, 0, 64, 20], [16, 16, 33, 33]], [[0, 48, 64, 16], [48, 0, 16, 64]]]


def test_graph_replayed_steps_follow_the_region_buffer(cuda, deterministic):
    """test_training_gpu.test_graph_replayed_steps_equal_eager_steps with `valid_region` in the batch, another one every step - before
    the capture, at the capture and in every replay.  A mask made on the host would freeze the capture's regions into the replays."""
    from boosted_detr_amd import engine
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD, CosineDecayRestarts
    from oracle import detr_oracle as O
    cfg, host = small_batch()
    params = O.make_params(cfg, seed=1)
    dev_batch = lambda b: {"image": to_device(b["image"]), "category": to_device(b["category"], torch.int32),
                           "attribute": to_device(b["attribute"], torch.int32), "bbox": to_device(b["bbox"]),
                           "num_objects": to_device(b["num_objects"], torch.int32)}
    batches = [dev_batch(host), dev_batch(small_batch(seed=21)[1])]
    kept = [R.token_keep(g, 64, 64, 2, 2).sum(1).tolist() for g in SMALL_REGIONS]
    assert all(min(k) >= 1 for k in kept) and len({str(k) for k in kept}) >= 4 and kept[2] != kept[4] != kept[6], kept
    regions = [to_device(np.asarray(g, np.int32), torch.int32) for g in SMALL_REGIONS]
    runs = {}
    keep_census, engine.SegmentedCapture.CENSUS = engine.SegmentedCapture.CENSUS, True
    try:
        for mode in ("eager", "graph", "no key"):
            m = small_model(dropout=0.1)
            m.compile(optimizer=SGD(CosineDecayRestarts(1e-3, 10, m_mul=.95, alpha=.1), momentum=.9, nesterov=True, clipnorm=.1))
            m.forward_backward(batches[0])
            m.set_weights_dict(params)
            m.use_graph = mode == "graph"
            steps = [dict(batches[i % 2], valid_region=regions[i]) if mode != "no key" else batches[i % 2] for i in range(8)]
            logs = [m.logs_to_host(m.train_step(s)) for s in steps]
            assert (len(m._graphs) == 1) == (mode == "graph") and m.steps_done == 8
            runs[mode] = (logs, m.get_weights_dict())
            if mode == "graph":
                census = m._graph_census              # SegmentedCapture.census() raised inside the capture on a memset / memcpy node
                assert census.get(0, 0) > 200 and not set(census) - set(engine.SegmentedCapture.ALLOWED_NODE_TYPES), census
                sig = next(iter(m._graphs))
                assert ("valid_region", (2, 4), torch.int32) in sig
                # a batch without the key is another signature: it never replays the masked capture
                assert m._graph_signature(batches[0]) not in m._graphs
    finally:
        engine.SegmentedCapture.CENSUS = keep_census
    (le, we), (lg, wg), (ln, wn) = runs["eager"], runs["graph"], runs["no key"]
    assert all(np.isfinite(l["loss"]) for l in lg)
    assert le == lg, (le, lg)                                                           # every logged value of every step, bit for bit
    bad = [k for k in we if not np.array_equal(we[k], wg[k])]
    assert not bad, bad[:5]
    assert all(a["loss"] != b["loss"] for a, b in zip(lg, ln))                          # the key was used in every step
    assert [k for k in we if not np.array_equal(we[k], wn[k])]


# ---------------------------------------------------------------- 6. Augmentations
def _injected_draw(aug, B, H, W):
    p = aug.draw(B, H, W)
    p.update(new_h=np.array([224, 120], np.int32), new_w=np.array([224, 150], np.int32),
             off_h=np.array([0, 16], np.int32), off_w=np.array([0, 0], np.int32))
    return p


def test_augmentations_emit_the_region_of_their_draw(detr_case):
    from boosted_detr_amd.pipeline import Augmentations
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    aug = Augmentations(seed=3, jpeg_quality=False, with_valid_region=True)
    p = _injected_draw(aug, 2, 224, 224)
    out = aug.apply(batch, p)
    region = out["valid_region"]
    assert isinstance(region, np.ndarray) and region.dtype == np.int32 and np.array_equal(region, R.MODEL_REGIONS)
    assert set(out) == set(batch) | {"valid_region"}
    plain = Augmentations(seed=3, jpeg_quality=False)
    assert set(plain.apply(batch, p)) == set(batch)                                     # default flag: the keys it always had
    drawn = aug.apply(batch)                                                            # ... and with its own draw the region fits the canvas
    g = drawn["valid_region"].astype(np.int64)
    assert (g[:, :2] >= 0).all() and (g[:, 2:] >= 1).all() and (g[:, 0] + g[:, 2] <= 224).all() and (g[:, 1] + g[:, 3] <= 224).all()
    model.set_weights_dict(params)
    model.forward_backward(out)                                                         # the model accepts the output
    logs = model.logs_to_host(model.step_logs())
    assert np.isfinite(logs["loss"])
    model.forward_backward(drawn)
    assert np.isfinite(model.logs_to_host(model.step_logs())["loss"])


# ---------------------------------------------------------------- 7. refusals, before any launch
GOOD = [0, 0, 224, 224]
BAD_HOST = {
    "shape [B,3]": np.zeros((2, 3), np.int32),
    "shape [3,4]": np.array([GOOD] * 3, np.int32),
    "dtype int64": np.array([GOOD, GOOD], np.int64),
    "top < 0": np.array([GOOD, [-1, 0, 100, 100]], np.int32),
    "left < 0": np.array([GOOD, [0, -1, 100, 100]], np.int32),
    "height < 1": np.array([GOOD, [10, 10, 0, 100]], np.int32),
    "width < 1": np.array([GOOD, [10, 10, 100, 0]], np.int32),
    "past the bottom": np.array([GOOD, [125, 0, 100, 100]], np.int32),
    "past the right": np.array([[0, 200, 100, 25], GOOD], np.int32),
    "no kept token": np.array([GOOD, [17, 17, 1, 1]], np.int32),
}


def test_bad_entries_raise_before_any_launch(detr_case, monkeypatch):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.engine import to_device
    cfg, batch, params, data, model, y_pred, out32, g32, out64, g64 = detr_case
    bad_device = {"shape [B,3]": to_device(np.zeros((2, 3), np.int32), torch.int32), "shape [3,4]": to_device(np.array([GOOD] * 3, np.int32), torch.int32),
                  "dtype int64": to_device(np.array([GOOD, GOOD]), torch.int64), "dtype float32": to_device(np.array([GOOD, GOOD], np.float32))}
    device_image = dict(batch, image=to_device(batch["image"]))
    torch.cuda.synchronize()

    def launched():
        raise AssertionError("a kernel was launched before the refusal")
    monkeypatch.setattr(K, "_stream", launched)          # every launch of kernels.py asks for its stream first
    for base in (batch, device_image):
        for what, region in list(BAD_HOST.items()) + list(bad_device.items()):
            for call in (lambda d: model.forward_backward(d), lambda d: model(d, training=False, raw=True), lambda d: model.predict_raw(d)):
                with pytest.raises(ValueError):
                    call(dict(base, valid_region=region))
    monkeypatch.undo()
    model.set_weights_dict(params)
    model.forward_backward(data)                         # the model is still in working order
    assert np.isfinite(model.logs_to_host(model.step_logs())["loss"])
