"""Training the panoptic mask head (DETR(train_panoptic_head=True)) at BASELINE.json configs[4]'s shapes, timed with events.

  head        PanopticAttention + PanopticNeck on a 25 x 42 x 256 image encoding, 300 queries, one head, dim 32: the forward alone
              and forward + backward (random mask gradient seeded on a Tape), batch 1 and 2, under the training step's 'split' policy
  step        the configs[4] training step (1333 x 800, ResNet-101, 6+6, 300 queries, batch 1) without and with train_panoptic_head

`python tools/panoptic_train_bench.py [head|step|all] [reps]`; prints one JSON line per measurement."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import numpy as np
import torch

what = sys.argv[1] if len(sys.argv) > 1 else "all"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def timed(fn, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def head(B):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd import panoptic_neck, transformers
    from boosted_detr_amd.engine import Tape, join_side_stream, recording
    g = torch.Generator(device="cuda").manual_seed(0)
    enc = torch.randn(B, 25, 42, 256, device="cuda", generator=g)
    dec = torch.randn(B, 300, 256, device="cuda", generator=g)
    pos = torch.randn(B, 25, 42, 256, device="cuda", generator=g)
    seed = torch.randn(B, 300, 529, device="cuda", generator=g)
    att = transformers.PanopticAttention(num_attention_heads=1, hidden_dim=32, seed=5)
    neck = panoptic_neck.PanopticNeck(seed=7)
    with K.gemm_precision("split"):
        neck([att([enc, dec, pos])])

        def fwd():
            return neck([att([enc, dec, pos])])

        def fwd_bwd():
            tape = Tape()
            with recording(tape):
                out = neck([att([enc, dec, pos])])
                tape.backward({id(out): seed})
                join_side_stream()

        f, fb = timed(fwd), timed(fwd_bwd)
    return {"what": f"panoptic head, configs[4] shapes, batch {B}", "forward_ms": round(f, 3), "forward_backward_ms": round(fb, 3),
            "backward_ms": round(fb - f, 3), "backward_over_forward": round((fb - f) / f, 2)}


def step(train_head):
    from bench import make_batch
    from boosted_detr_amd import parameters
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.model import DETR
    from boosted_detr_amd.training import SGD, CosineDecayRestarts
    model = DETR(num_object_preds=300, image_size=(800, 1333), num_encoder_blocks=6, num_encoder_heads=8, encoder_dim=256,
                 num_decoder_blocks=6, num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32,
                 vocab_dict=parameters.COCO_VOCAB, attribute_weight=0.0, backbone_name="ResNet101", train_panoptic_head=train_head)
    model.compile(optimizer=SGD(CosineDecayRestarts(1e-3, 4000, m_mul=0.95, alpha=0.1), momentum=0.9, nesterov=True, clipnorm=0.1))
    host = make_batch(1, 800, 1333, 300, 80, seed=0)
    if train_head:
        host["masks"] = (np.random.default_rng(1).random((1, 300, 23, 23)) > 0.6).astype(np.float32)
    batch = {k: to_device(v, torch.int32 if v.dtype == np.int32 else torch.float32) for k, v in host.items()}
    ms = timed(lambda: model.train_step(batch))
    logs = model.logs_to_host(model.train_step(batch))
    return {"what": "configs[4] training step, batch 1" + (" + train_panoptic_head" if train_head else ""), "step_ms": round(ms, 3),
            "loss": logs["loss"], "Mask_Loss": logs.get("Mask_Loss")}


if what in ("all", "head"):
    for B in (1, 2):
        print(json.dumps(head(B)), flush=True)
if what in ("all", "step"):
    for train_head in (False, True):
        print(json.dumps(step(train_head)), flush=True)
