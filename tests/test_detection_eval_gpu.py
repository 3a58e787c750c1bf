"""GPU half of the detection metric: bdetr_det_postprocess / bdetr_det_match against the plain-loop fp64 reference (tests/_ap_ref.py),
bit for bit (order, label, score, tp_bits, matched_gt, gt_count), and Model.evaluate / detections / DetectionAP end to end."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _ap_ref as R

pytestmark = pytest.mark.gpu

THR10 = np.linspace(0.5, 0.95, 10)


def make_case(seed, B, N, M, C, num_objects, max_dets=100, score_levels=None, crowded_class=None):
    """Ground truths at random; most detections are jittered copies of a ground truth of their image (IoUs spread over the
    thresholds), labelled like it or at random."""
    rng = np.random.default_rng(seed)
    gt_box = np.concatenate([rng.uniform(0.0, 0.6, (B, M, 2)), rng.uniform(0.05, 0.4, (B, M, 2))], -1).astype(np.float32)
    gt_label = rng.integers(2, C, (B, M)).astype(np.int32)
    if crowded_class is not None:
        gt_label[:, : M // 2] = crowded_class
    src = rng.integers(0, M, (B, N))
    box = np.take_along_axis(gt_box, src[..., None], 1) + rng.normal(0, 0.03, (B, N, 4)).astype(np.float32)
    label = np.take_along_axis(gt_label, src, 1)
    swap = rng.random((B, N)) < 0.25
    label = np.where(swap, rng.integers(2, C, (B, N)), label).astype(np.int32)
    if crowded_class is not None:
        label[:, : (2 * N) // 3] = crowded_class
    score = (rng.random((B, N), dtype=np.float32) if score_levels is None else rng.choice(score_levels, (B, N))).astype(np.float32)
    return {"score": score, "label": label, "box": box.astype(np.float32), "gt_label": gt_label, "gt_box": gt_box,
            "num_objects": np.asarray(num_objects, np.int32), "C": C, "thresholds": THR10, "max_dets": max_dets}


def edge_cases():
    cases = {}
    cases["random_B3_N50_M20"] = make_case(1, 3, 50, 20, 8, [0, 20, 7])
    cases["off_wave_N37_M5"] = make_case(2, 2, 37, 5, 6, [5, 3])
    cases["truncation_N300_M100"] = make_case(3, 1, 300, 100, 8, [100], max_dets=100, crowded_class=3)
    cases["duplicated_scores"] = make_case(4, 2, 50, 20, 5, [20, 11], score_levels=[0.125, 0.25, 0.5, 0.7])

    c = make_case(5, 2, 37, 12, 5, [12, 12])                     # duplicated ground truths: rows 2k and 2k+1 are the same object
    c["gt_box"][:, 1::2], c["gt_label"][:, 1::2] = c["gt_box"][:, 0::2], c["gt_label"][:, 0::2]
    c["box"][:, :6], c["label"][:, :6] = c["gt_box"][:, 0:12:2], c["gt_label"][:, 0:12:2]      # six detections sit exactly on a pair
    c["score"][:, :6] = 0.99
    cases["duplicated_gt_boxes"] = c

    g = np.asarray([[0.0, 0.0, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5]], np.float32)       # dyadic: IoU = 1/2 and 3/4 exactly
    d = np.asarray([[0.0, 0.0, 0.5, 0.25], [0.5, 0.5, 0.5, 0.375], [0.0, 0.0, 0.25, 0.25]], np.float32)      # IoU 0.5, 0.75, 0.25
    cases["iou_equals_threshold"] = {"score": np.asarray([[0.9, 0.8, 0.7]], np.float32), "label": np.full((1, 3), 2, np.int32), "box": d[None],
                                     "gt_label": np.full((1, 2), 2, np.int32), "gt_box": g[None], "num_objects": np.asarray([2], np.int32),
                                     "C": 3, "thresholds": np.asarray([0.25, 0.5, 0.75]), "max_dets": 100}

    c = make_case(6, 2, 37, 8, 5, [8, 8])                        # zero and negative extents on both sides
    c["box"][:, 0:4, 2], c["box"][:, 4:8, 3] = 0.0, -0.3
    c["gt_box"][:, 0, 2], c["gt_box"][:, 1, 3] = 0.0, -0.2
    c["box"][:, 8], c["label"][:, 8] = c["gt_box"][:, 0], c["gt_label"][:, 0]      # a detection ON the degenerate ground truths
    c["box"][:, 9], c["label"][:, 9] = c["gt_box"][:, 1], c["gt_label"][:, 1]
    cases["zero_and_negative_extents"] = c

    c = make_case(7, 2, 37, 10, 5, [4, 0])                       # rows past num_objects: the -10 padding, and a tempting row to ignore
    c["gt_box"][0, 4:], c["gt_box"][1, :] = -10.0, -10.0
    c["gt_box"][0, 9], c["gt_label"][0, 9] = c["box"][0, 0], c["label"][0, 0]      # matches detection 0 perfectly, but does not exist
    cases["padding_rows"] = c

    c = make_case(8, 2, 37, 10, 5, [10, 10])                     # <PAD> / <OOV> among the real rows, and a label beyond the vocabulary
    c["gt_label"][:, 0], c["gt_label"][:, 1], c["gt_label"][1, 2] = 0, 1, 5
    c["label"][:, 0], c["box"][:, 0] = 1, c["gt_box"][:, 1]      # (a caller's own label 1 still finds no <OOV> ground truth)
    cases["ignored_ground_truth_ids"] = c
    return cases


CASES = edge_cases()
_REF = {}


def reference(name):
    """The reference's answer for a case, computed once and shared."""
    if name not in _REF:
        c = CASES[name]
        _, images = R.evaluate([{k: c[k] for k in ("score", "label", "box", "gt_label", "gt_box", "num_objects")}],
                               c["thresholds"], c["max_dets"], c["C"])
        _REF[name] = images
    return _REF[name]


def run_match(c, gt_count=None):
    from boosted_detr_amd import kernels as K
    dev = "cuda"
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("score", "label", "box", "gt_label", "gt_box", "num_objects")}
    if gt_count is None:
        gt_count = torch.zeros(c["C"], dtype=torch.int32, device=dev)
    order, tp_bits, matched = K.det_match(t["score"], t["label"], t["box"], t["gt_label"], t["gt_box"], t["num_objects"], c["thresholds"],
                                          c["C"], c["max_dets"], gt_count)
    torch.cuda.synchronize()
    return order.cpu().numpy(), tp_bits.cpu().numpy().view(np.uint16), matched.cpu().numpy(), gt_count


@pytest.mark.parametrize("name", list(CASES))
def test_match_bit_exact(cuda, name):
    c, images = CASES[name], reference(name)
    order, tp_bits, matched, gt_count = run_match(c)
    want_count = sum(im["gt_count"] for im in images)
    for b, im in enumerate(images):
        assert np.array_equal(order[b], im["order"]), (name, b, "order")
        assert np.array_equal(tp_bits[b], R.pack_bits(im["keep"], im["tp"])), (name, b, "tp_bits")
        assert np.array_equal(matched[b], im["matched_gt"]), (name, b, "matched_gt")
    assert np.array_equal(gt_count.cpu().numpy(), want_count), name
    # each case exercises what it is there for (properties of the reference's answer, so of the kernel's too)
    keep = np.stack([im["keep"] for im in images])
    tp = np.stack([im["tp"] for im in images])
    if name == "truncation_N300_M100":
        assert (c["label"] == 3).sum() > 100 and (~keep).sum() == (c["label"] == 3).sum() - 100 and keep[c["label"] != 3].all()
    else:
        assert keep.all()
    if name in ("random_B3_N50_M20", "off_wave_N37_M5", "truncation_N300_M100", "duplicated_scores"):
        assert tp[:, 0].any() and not tp[:, 0].all() and tp[:, 0].sum() > tp[:, -1].sum()
    if name == "random_B3_N50_M20":
        assert not tp[0].any() and (matched[0] == -1).all()                       # num_objects = 0
    if name == "duplicated_scores":
        assert len(np.unique(c["score"])) == 4
    if name == "duplicated_gt_boxes":
        assert (matched[:, :, :6] == np.arange(1, 12, 2)[None, None, :]).all()    # equal IoU: the larger index of each pair
    if name == "iou_equals_threshold":
        assert tp_bits[0].tolist() == [0x8000 | 0b011, 0x8000 | 0b111, 0x8000]    # IoU 0.5 and 0.75 meet their thresholds; 0.25's object is taken
    if name == "zero_and_negative_extents":
        assert (matched[:, :, :10] == -1).all()
    if name == "padding_rows":
        assert (matched != 9).all() and (matched[1] == -1).all() and want_count.sum() == 4
    if name == "ignored_ground_truth_ids":
        assert want_count[:2].sum() == 0 and want_count.sum() == 20 - 5 and (matched[:, :, 0] == -1).all() and not np.isin(matched, [0, 1]).any()


def test_gt_count_accumulates_across_calls(cuda):
    c = CASES["off_wave_N37_M5"]
    _, _, _, gt_count = run_match(c)
    once = gt_count.cpu().numpy().copy()
    run_match(c, gt_count)
    assert np.array_equal(gt_count.cpu().numpy(), 2 * once) and once.sum() == 8


def test_postprocess_matches_numpy(cuda):
    from boosted_detr_amd import kernels as K
    rng = np.random.default_rng(11)
    logits = rng.normal(0, 2, (3, 37, 11)).astype(np.float32)
    p = np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)
    p = p.astype(np.float32)
    p[0, :10] = np.round(p[0, :10] * 8) / 8              # ties: the first maximum wins
    p[1, :10, 0], p[1, 10:20, 1] = 0.99, 0.99            # <PAD> / <OOV> most probable: still never the label
    p[2, 0, 2:] = 0.0625                                 # all equal
    score, label = K.det_postprocess(torch.from_numpy(p).cuda())
    torch.cuda.synchronize()
    want_label = p[..., 2:].argmax(-1) + 2
    assert np.array_equal(label.cpu().numpy(), want_label) and label.dtype == torch.int32
    assert np.array_equal(score.cpu().numpy().view(np.uint32), np.take_along_axis(p, want_label[..., None], -1)[..., 0].view(np.uint32))
    ref_score, ref_label = R.postprocess(p)
    assert np.array_equal(ref_label, want_label) and np.array_equal(ref_score, score.cpu().numpy())
    assert (p[0, :10, 2:] == p[0, :10, 2:].max(-1, keepdims=True)).sum(-1).max() > 1      # the ties exist


@pytest.mark.parametrize("over", [dict(N=1025), dict(M=1025), dict(T=16), dict(T=0), dict(C=2), dict(max_dets=0)])
def test_over_limit_shapes_are_refused_without_a_launch(cuda, over):
    from boosted_detr_amd import _lib
    N, M, T, C, max_dets = (over.get(k, v) for k, v in (("N", 8), ("M", 4), ("T", 3), ("C", 5), ("max_dets", 100)))
    dev = "cuda"
    score, label, box = torch.rand(1, N, device=dev), torch.full((1, N), 2, dtype=torch.int32, device=dev), torch.rand(1, N, 4, device=dev)
    gl, gb = torch.full((1, M), 2, dtype=torch.int32, device=dev), torch.rand(1, M, 4, device=dev)
    nobj = torch.full((1,), M, dtype=torch.int32, device=dev)
    order = torch.full((1, N), -7, dtype=torch.int32, device=dev)
    tpb = torch.full((1, N), -7, dtype=torch.int16, device=dev)
    matched = torch.full((1, max(T, 1), N), -7, dtype=torch.int32, device=dev)
    count = torch.zeros(max(C, 3), dtype=torch.int32, device=dev)
    thr = np.linspace(0.5, 0.95, max(T, 1))
    st = _lib.lib().bdetr_det_match(score.data_ptr(), label.data_ptr(), box.data_ptr(), gl.data_ptr(), gb.data_ptr(), nobj.data_ptr(),
                                    thr.ctypes.data, 1, N, M, C, T, max_dets, order.data_ptr(), tpb.data_ptr(), matched.data_ptr(),
                                    count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == -1 and b"bdetr_det_match" in _lib.lib().bdetr_last_error()
    torch.cuda.synchronize()
    assert (order == -7).all() and (tpb == -7).all() and (matched == -7).all() and (count == 0).all()      # nothing ran
    with pytest.raises(_lib.BdetrError):
        _lib.check(st, "det_match")
    if "C" in over:
        st = _lib.lib().bdetr_det_postprocess(score.data_ptr(), 1, N, C, score.data_ptr(), label.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == -1


def test_known_answers_through_the_kernels(cuda):
    """The hand-derived cases of tests/golden/detection_ap_kats.json through DetectionEvaluator.update / result."""
    from boosted_detr_amd.evaluation import DetectionEvaluator
    for case in json.loads((Path(__file__).parent / "golden" / "detection_ap_kats.json").read_text())["cases"]:
        C = case["num_classes"]
        ev = DetectionEvaluator(C, case["thresholds"], case["max_dets"])
        for im in case["images"]:
            cat_pred = np.zeros((1, len(im["score"]), C), np.float32)
            cat_pred[0, np.arange(len(im["score"])), im["label"]] = im["score"]
            ev.update(torch.from_numpy(cat_pred).cuda(), torch.tensor([im["box"]], dtype=torch.float32).cuda(),
                      torch.tensor([im["gt_label"]], dtype=torch.int32).cuda(), torch.tensor([im["gt_box"]], dtype=torch.float32).cuda(),
                      torch.tensor([im["num_objects"]], dtype=torch.int32).cuda())
        res = ev.result()
        for k in ("AP", "AP50", "AP75", "AR"):
            want = case["expected"][k]
            assert (math.isnan(res[k]) if want is None else abs(res[k] - want) <= 1e-12), (case["name"], k, res[k])
        assert res["gt_count"].tolist() == case["expected"]["gt_count"]


# ---------------------------------------------------------------------------------------------------------------------
# end to end at BASELINE.json configs[0]: 2 x 224 x 224, 1 + 1 blocks, 50 queries, seeded weights, two batches
# ---------------------------------------------------------------------------------------------------------------------
def build_model(cfg, image_size=None):
    from boosted_detr_amd import parameters, transformers
    from boosted_detr_amd.model import DETR
    transformers.AttentionBlock.dropout_rate = 0.0
    transformers.FeedForwardBlock.dropout_rate = 0.0
    return DETR(num_object_preds=cfg.num_object_preds, image_size=cfg.image_size, num_encoder_blocks=cfg.num_encoder_blocks,
                num_encoder_heads=cfg.num_encoder_heads, encoder_dim=cfg.encoder_dim, num_decoder_blocks=cfg.num_decoder_blocks,
                num_decoder_heads=cfg.num_decoder_heads, decoder_dim=cfg.decoder_dim, num_panoptic_heads=1, panoptic_dim=32,
                vocab_dict=parameters.synthetic_vocab(cfg.num_categories - 2, cfg.num_attributes - 2), attribute_weight=cfg.attribute_weight)


def state_of(model):
    opt = model.optimizer
    tensors = {v.name: v.value.detach().clone() for v in model.variables}
    tensors.update({f"slot/{k}": t.detach().clone() for k, t in opt.flat_slots.items()})
    return tensors, (opt.iterations, model.steps_done, model._step_seed(), len(model._graphs), len(model.trainable_variables))


@pytest.fixture(scope="module")
def trained(cuda):
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    cfg = O.CONFIG1
    batches = [O.make_batch(cfg, 2, 20, seed=1234, num_objects=[3, 7]), O.make_batch(cfg, 2, 20, seed=4321, num_objects=[5, 0])]
    model = build_model(cfg)
    model.compile(optimizer=SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1))
    model.forward_backward(batches[0])                     # build-by-first-call
    model.set_weights_dict(O.make_params(cfg, seed=0))
    model.train_step(batches[0])
    # seeded weights find nothing: make some of the second batch's objects the model's own detections, so that AP is not trivially 0
    det = model.detections(batches[1])
    boxes, labels = det["boxes"].cpu().numpy(), det["labels"].cpu().numpy()
    batches[1]["bbox"][0, :5], batches[1]["category"][0, :5] = boxes[0, 10:15], labels[0, 10:15]
    torch.cuda.synchronize()
    return cfg, batches, model


def test_evaluate_end_to_end(trained):
    cfg, batches, model = trained
    before = state_of(model)
    res = model.evaluate(batches)
    again = model.evaluate(batches)
    torch.cuda.synchronize()
    after = state_of(model)
    assert before[1] == after[1]
    assert set(before[0]) == set(after[0]) and len(before[0]) > 100
    for k, t in before[0].items():
        assert torch.equal(t, after[0][k]), k               # weights, moving statistics, optimizer slots: bit-identical
    for k in ("AP", "AP50", "AP75", "AR"):
        assert res[k] == again[k]
    assert np.array_equal(res["per_class_AP"], again["per_class_AP"], equal_nan=True) and np.array_equal(res["gt_count"], again["gt_count"])

    ref_batches = []
    for b in batches:
        cat, _, box = model.predict_raw(b)
        score, label = R.postprocess(cat.cpu().numpy())
        ref_batches.append({"score": score, "label": label, "box": box.cpu().numpy(), "gt_label": b["category"], "gt_box": b["bbox"],
                            "num_objects": b["num_objects"]})
    ref, _ = R.evaluate(ref_batches, THR10, 100, cfg.num_categories)
    for k in ("AP", "AP50", "AP75", "AR"):
        assert abs(res[k] - ref[k]) <= 1e-12, (k, res[k], ref[k])
    valid = res["gt_count"] > 0
    assert np.abs(res["per_class_AP"][valid] - ref["per_class_AP"][valid]).max() <= 1e-12
    assert res["AP"] > 0.0 and res["num_images"] == 4 and res["num_detections"] == 4 * 50 and res["num_ground_truths"] == 15
    assert model.evaluate(batches, return_dict=False) == [res[k] for k in ("AP", "AP50", "AP75", "AR")]
    assert model.evaluate(batches, steps=1)["num_images"] == 2

    it = model.optimizer.iterations                          # and training goes on as if nothing had happened
    logs = model.logs_to_host(model.train_step(batches[0]))
    assert math.isfinite(logs["loss"]) and model.optimizer.iterations == it + 1


def test_detections_agree_with_inverse_tokenization(trained):
    cfg, batches, model = trained
    cat, att, box = model.predict_raw(batches[0])
    assert cat.is_cuda and tuple(cat.shape) == (2, 50, cfg.num_categories) and tuple(box.shape) == (2, 50, 4)
    det = model.detections(batches[0])
    ids, _ = model.InverseTokenization.token_ids(cat, att)
    labels = det["labels"].cpu().numpy()
    assert (labels >= 2).all() and np.array_equal(labels[ids >= 2], ids[ids >= 2])
    assert torch.equal(det["boxes"], box) and torch.equal(det["scores"], cat.gather(2, det["labels"].long()[..., None])[..., 0])
    words, _, boxes = model(batches[0], training=False)      # the decoded path is what it was
    assert words.shape == (2, 50, 1) and words[0, 0, 0] == model.InverseTokenization._cat_vocab[ids[0, 0]] and torch.equal(boxes, box)


def test_fit_with_detection_ap_logs_validation_keys(cuda):
    from boosted_detr_amd.training import SGD, Callback, DetectionAP
    from oracle import detr_oracle as O
    cfg = O.Config(image_size=(64, 64), num_object_preds=10, num_decoder_blocks=2, num_categories=12, num_attributes=6)
    batch = O.make_batch(cfg, 2, 5, seed=9, num_objects=[2, 4])
    model = build_model(cfg)
    model.compile(optimizer=SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1))
    seen = []

    class Record(Callback):
        def on_epoch_end(self, epoch, logs=None):
            seen.append(dict(logs))

    model.fit([batch] * 2, epochs=1, callbacks=[DetectionAP([batch]), Record()], verbose=0)
    assert len(seen) == 1 and model.optimizer.iterations == 2
    for k in ("val_AP", "val_AP50", "val_AP75", "val_AR"):
        assert 0.0 <= seen[0][k] <= 1.0, (k, seen[0])
    assert "loss" in seen[0]
