"""The cost of DETR's auxiliary decoder losses (DETR(use_intermediate_losses=True)) at BASELINE.json configs[1]'s shapes (640 x 640,
ResNet-50, 6 + 6 layers, 100 queries, batch 16), three training steps side by side in ONE process:

  off       the option off (the step bench.py times)
  looped    the option on, BDETR_AUX_STACKED=0: heads, matcher and loss per decoder block over the existing kernels
  stacked   the option on, default: one pass of heads / matcher / loss over the six blocks' outputs stacked

Each variant is its own model (same seed), warmed up and captured (Model.use_graph); the timed rounds then alternate between the variants
(off, looped, stacked, off, ...) so that clock or thermal drift hits all three alike, and the figure per variant is the MEDIAN over the
rounds of the event-timed mean step.  The launch count is the number of kernel nodes in each variant's captured step
(engine.SegmentedCapture.census), not an estimate.  A second table times the same steps enqueued eagerly from Python.

`python tools/aux_loss_bench.py [rounds] [steps per round]`; prints one JSON line per variant and mode, then a summary line."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
VARIANTS = (("off", False, "1"), ("looped", True, "0"), ("stacked", True, "1"))


def build(aux, stacked_env):
    from bench import make_batch
    from boosted_detr_amd import parameters
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.model import DETR
    from boosted_detr_amd.training import SGD, CosineDecayRestarts
    keep = os.environ.get("BDETR_AUX_STACKED")
    os.environ["BDETR_AUX_STACKED"] = stacked_env
    try:
        model = DETR(num_object_preds=100, image_size=(640, 640), num_encoder_blocks=6, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=6,
                     num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32, vocab_dict=parameters.COCO_VOCAB, attribute_weight=0.0,
                     use_intermediate_losses=aux)
    finally:
        if keep is None:
            del os.environ["BDETR_AUX_STACKED"]
        else:
            os.environ["BDETR_AUX_STACKED"] = keep
    model.compile(optimizer=SGD(CosineDecayRestarts(1e-3, 4000, m_mul=0.95, alpha=0.1), momentum=0.9, nesterov=True, clipnorm=0.1))
    host = make_batch(16, 640, 640, 100, 80, seed=0)
    batch = {k: to_device(v, torch.int32 if v.dtype == np.int32 else torch.float32) for k, v in host.items()}
    return model, batch


def timed(model, batch, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        model.train_step(batch)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    from boosted_detr_amd import engine
    engine.SegmentedCapture.CENSUS = True
    models = {}
    for name, aux, env in VARIANTS:
        model, batch = build(aux, env)
        model.use_graph = True
        for _ in range(6):                       # build-by-first-call, two eager steps on the signature, the capture, replays
            model.train_step(batch)
        model.guard_flush()
        torch.cuda.synchronize()
        assert len(model._graphs) == 1, "the step was not captured"
        models[name] = (model, batch)
    result = {}
    for mode in ("graph", "eager"):
        per = {name: [] for name in models}
        for name, (model, batch) in models.items():
            model.use_graph = mode == "graph"
            timed(model, batch, 3)               # warm-up in this mode
        for _ in range(rounds if mode == "graph" else max(3, rounds // 2)):
            for name, (model, batch) in models.items():
                per[name].append(timed(model, batch, steps))
        for name, (model, batch) in models.items():
            census = model._graph_census or {}
            logs = model.logs_to_host(model.train_step(batch))
            row = {"variant": name, "mode": mode, "step_ms_median": round(statistics.median(per[name]), 3), "step_ms_min": round(min(per[name]), 3),
                   "step_ms_max": round(max(per[name]), 3), "rounds": len(per[name]), "steps_per_round": steps,
                   "kernel_launches_per_step": int(sum(census.values())), "loss": round(logs["loss"], 4)}
            result[(name, mode)] = row
            print(json.dumps(row), flush=True)
    summary = {"what": "auxiliary decoder losses at configs[1] shapes (batch 16, 6 decoder blocks)"}
    for mode in ("graph", "eager"):
        off, looped, stacked = (result[(n, mode)]["step_ms_median"] for n in ("off", "looped", "stacked"))
        summary[mode] = {"stacked_minus_off_ms": round(stacked - off, 3), "looped_minus_off_ms": round(looped - off, 3),
                         "stacked_minus_looped_ms": round(stacked - looped, 3)}
    launches = {n: result[(n, "graph")]["kernel_launches_per_step"] for n in ("off", "looped", "stacked")}
    summary["launches_added"] = {"stacked": launches["stacked"] - launches["off"], "looped": launches["looped"] - launches["off"]}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
