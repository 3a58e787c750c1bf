"""In deterministic mode a training step's result is independent of the stream schedule.  Every model below runs its
steps once in stream order (side stream off: the reference) and then with the side stream on under four schedules - unperturbed, a
backlogged main stream, a late side stream, both (tests/_schedule.py) - and every loss and every weight must equal the reference bit
for bit.  The toy steps are bound by host enqueue time, so without the forced schedules the two streams are serialised by the host
and a missing fork wait, a missing join, an operand freed too early or overwritten in place would go unseen; a leg whose schedule
did not materialise fails."""
import numpy as np
import pytest
import torch

import _schedule as S
from test_training_gpu import deterministic, small_batch, small_model  # noqa: F401  (deterministic is a fixture)

pytestmark = pytest.mark.gpu

# the smallest image at which every in-place path counter of the 'split' leg is non-zero (test_detr_eager_steps[split] asserts them)
IMAGE = 64


def _device_batch(host):
    from boosted_detr_amd.engine import to_device
    out = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
           "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    if "masks" in host:
        out["masks"] = to_device(host["masks"])
    return out


def _sgd():
    from boosted_detr_amd.training import SGD
    return SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1)


def _toy():
    """(params, two device batches) of the 64 x 64 toy problem, B = 2."""
    from oracle import detr_oracle as O
    cfg, host = small_batch()
    return O.make_params(cfg, seed=1), [_device_batch(host), _device_batch(small_batch(seed=21)[1])]


def _detr_builder(params, batches, optimizer=_sgd, policy=None, graph=False, **kw):
    def build():
        m = small_model(dropout=0.1, **kw)
        m.compile(optimizer=optimizer())
        if policy is not None:
            m.train_gemm_precision = policy
        m.forward_backward(batches[0])
        m.set_weights_dict(params)
        m.use_graph = graph
        return m
    return build


def _check(legs, problems, steps):
    ref = legs["reference"]
    assert len(ref[0]) == steps and all(np.isfinite(ref[0])) and len(ref[1]) > 100, ref[0]
    assert len(set(ref[0])) > 1                                        # the steps differ from each other: masks, batches and weights move
    assert not problems, "\n".join(problems)
    for kind in S.SCHEDULES[1:]:
        assert legs[kind][2]["side_tasks"] > 0 and legs[kind][2]["range_redos"] == 0, (kind, legs[kind][2])


@pytest.mark.parametrize("policy", ["mixed", "split"])
def test_detr_eager_steps(cuda, deterministic, policy):  # noqa: F811
    """DETR, SGD with momentum, Nesterov and clipnorm, dropout 0.1, three eager steps.  Under 'split' the backward pass runs the
    in-place epilogues the schedules are after: each must have been reached."""
    params, batches = _toy()
    legs, problems = S.run_all_legs(_detr_builder(params, batches, policy=policy), batches, 3)
    _check(legs, problems, 3)
    if policy == "split":
        for kind in S.SCHEDULES:
            c = legs[kind][2]
            assert c["masked_accum"] >= 1 and c["bwd_data_accumulate"] >= 1 and c["lazy_skip"] >= 1, (IMAGE, kind, c)
            assert c["tape_relu_mask_apply"] + c["tape_axpy"] >= 1, (IMAGE, kind, c)


def test_detr_graph_replays(cuda, deterministic):  # noqa: F811
    """The same DETR through use_graph: eight steps, five of them replays (the first builds the optimizer's buffers, which changes the
    step's signature; the fourth is the third on the final signature: it captures, and replays what it captured).  The schedules hit
    the replays - SegmentedCapture.replay forks and joins at segment granularity - and the eager steps in front; against eight
    eager stream-ordered steps."""
    params, batches = _toy()
    legs, problems = S.run_all_legs(_detr_builder(params, batches, graph=True), batches, 8, build_reference=_detr_builder(params, batches))
    _check(legs, problems, 8)
    assert legs["reference"][2]["graphs"] == 0
    for kind in S.SCHEDULES[1:]:
        rep = legs[kind][2]["schedule"]
        assert legs[kind][2]["graphs"] == 1 and rep["exempt"] == [0, 3], (kind, legs[kind][2]["graphs"], rep["exempt"])


def test_boosted_three_learners(cuda, deterministic):  # noqa: F811
    """BoostedDETR with three learners: the shared queries take the temporary-gradient sink, an axpy_ inside side tasks."""
    from oracle import detr_oracle as O
    from test_model_gpu import build_model
    cfg = O.Config(image_size=(64, 64), num_object_preds=10, num_decoder_blocks=3, boosted=True, num_categories=12, num_attributes=6)
    params = O.make_params(cfg, seed=1)
    batches = [_device_batch(O.make_batch(cfg, 2, 5, seed=s, num_objects=[2, 4])) for s in (9, 21)]

    def build():
        m = build_model(cfg, boosted=True, dropout=0.1)
        m.compile(optimizer=_sgd())
        m.forward_backward(batches[0])
        m.set_weights_dict(params)
        return m

    legs, problems = S.run_all_legs(build, batches, 3)
    _check(legs, problems, 3)
    assert all(legs[kind][2]["sink_axpy"] >= 1 for kind in S.SCHEDULES), {k: legs[k][2]["sink_axpy"] for k in legs}


def test_trainable_panoptic_head_with_stacked_aux_losses(cuda, deterministic):  # noqa: F811
    """Panoptic head trainable and auxiliary decoder losses stacked: the panoptic_neck side tasks, the grouped heads, grouped BatchNorm."""
    from boosted_detr_amd import parameters, transformers
    from boosted_detr_amd.model import DETR
    from test_panoptic_train_gpu import _small_head_batch
    batches = [_small_head_batch(9), _small_head_batch(21)]
    start = {}

    def build():
        m = DETR(num_object_preds=30, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=2,
                 num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32, vocab_dict=parameters.synthetic_vocab(10, 4),
                 attribute_weight=1.0, train_panoptic_head=True, use_intermediate_losses=True)
        transformers.AttentionBlock.dropout_rate = transformers.FeedForwardBlock.dropout_rate = 0.1
        m.compile(optimizer=_sgd())
        m.forward_backward(batches[0])
        if not start:                         # every leg starts from the weights the first (stream-ordered) build left
            start.update(m.get_weights_dict())
        m.set_weights_dict(start)
        return m

    legs, problems = S.run_all_legs(build, batches, 3)
    _check(legs, problems, 3)


def test_backbone_frozen_between_steps(cuda, deterministic):  # noqa: F811
    """EncoderBackbone.trainable = False after two steps: gradients the frozen layers drop on the side stream, and the optimizer's
    flat buffers rebuilt in front of the next step."""
    params, batches = _toy()

    def freeze(model, i):
        if i == 2:
            model.EncoderBackbone.trainable = False

    legs, problems = S.run_all_legs(_detr_builder(params, batches), batches, 5, each_step=freeze)
    _check(legs, problems, 5)
    first = next(k for k in sorted(params) if k.startswith("EncoderBackbone") and k.endswith("kernel"))
    assert not np.array_equal(legs["reference"][1][first], np.asarray(params[first]))      # (it trained before the freeze)


def test_detr_adamw(cuda, deterministic):  # noqa: F811
    """AdamW instead of SGD: the fused multi-tensor step reads the flat gradient buffer right behind the join."""
    from boosted_detr_amd.training import AdamW
    params, batches = _toy()
    legs, problems = S.run_all_legs(_detr_builder(params, batches, optimizer=lambda: AdamW(1e-3, weight_decay=1e-4, clipnorm=.1)), batches, 3)
    _check(legs, problems, 3)
