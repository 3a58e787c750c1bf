"""SHA-256 digests of whole training steps on the seeded toy problem of tests/test_training_gpu.py (64x64 image, 10 queries, 1 encoder
and 2 decoder blocks, batch 2, weights O.make_params(cfg, seed=1)) in deterministic mode: every per-step loss vector and all weights
after the last step of (a) eight eager steps, (b) the same through Model.use_graph, (c) three overflowing steps under the 'split'
policy that the range guard redoes.  Used by tests/golden/make_step_parent_digests.py (recorded from the commit before the step
control of training.Model was split into objects of their own) and by the test that requires the current tree to reproduce them."""
import hashlib

import numpy as np
import torch

from test_training_gpu import small_batch, small_model

OVERFLOWING = "EncoderBackbone/resnet50/conv2_block1_1_bn/beta"


def _sha(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _weights(model) -> str:
    w = model.get_weights_dict()
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    return h.hexdigest()


def _loss(logs) -> str:
    return _sha(t.detach().cpu().numpy() for t in logs["loss"])      # (a host read per step: a replay returns the captured tensors)


def step_digests() -> dict:
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.training import SGD, CosineDecayRestarts
    from oracle import detr_oracle as O
    cfg, host = small_batch()
    hosts = [host, small_batch(seed=21)[1]]
    params = O.make_params(cfg, seed=1)
    out = {"inputs": _sha([params[k] for k in sorted(params)] + [np.asarray(b[k]) for b in hosts for k in sorted(b)])}
    dev_batch = lambda b: {"image": to_device(b["image"]), "category": to_device(b["category"], torch.int32),
                           "attribute": to_device(b["attribute"], torch.int32), "bbox": to_device(b["bbox"]),
                           "num_objects": to_device(b["num_objects"], torch.int32)}
    batches = [dev_batch(b) for b in hosts]
    prev = K.set_deterministic(True)
    try:
        for leg, graph in (("eager", False), ("graph", True)):
            m = small_model(dropout=0.1)
            m.compile(optimizer=SGD(CosineDecayRestarts(1e-3, 10, m_mul=.95, alpha=.1), momentum=.9, nesterov=True, clipnorm=.1))
            m.forward_backward(batches[0])
            m.set_weights_dict(params)
            m.use_graph = graph
            losses = [_loss(m.train_step(batches[i % 2])) for i in range(8)]
            assert (len(m._graphs) == 1) == graph and m.steps_done == 8 and m.optimizer.iterations == 8      # capture on the third step, five replays
            out[leg] = {"losses": losses, "weights": _weights(m)}
        # (c) the overflow case of test_range_guard_redoes_an_overflowing_step_on_the_fp32_forward, lagged: nothing is resolved at once
        bad = dict(params)
        bad[OVERFLOWING] = np.full_like(params[OVERFLOWING], 1e5)
        K.read_and_clear_overflow()
        m = small_model()
        m.compile(optimizer=SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1))
        m.train_gemm_precision = "mixed"
        m.forward_backward(host)
        m.set_weights_dict(bad)
        m.train_gemm_precision = "split"
        assert m.GUARD_LAG == 2
        losses = [_loss(m.train_step(host)) for _ in range(3)]
        flushed = m.guard_flush()
        out["redo"] = {"losses": losses, "weights": _weights(m), "flushed": flushed is not None, "range_redos": m.range_redos,
                       "range_skipped": m.range_skipped, "steps_done": m.steps_done, "iterations": m.optimizer.iterations}
        K.read_and_clear_overflow()
    finally:
        K.set_deterministic(prev)
    return out
