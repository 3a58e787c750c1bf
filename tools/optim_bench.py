"""Time the two fused multi-tensor optimizer entry points (csrc/optim.hip) on the variable list of BASELINE.json configs[1]
(31.0 M trainable parameters): bdetr_sgd_nesterov_clipnorm and bdetr_adamw_clipnorm, alternating in one process, each launch between
two device events.  Prints per-launch microseconds and achieved bytes/s; the byte counts come from the sizes:

    SGD   24 B / element: norm pass reads g (4), apply reads g, v, w (12) and writes v, w (8)
    AdamW 32 B / element: norm pass reads g (4), apply reads g, m, v, w (16) and writes m, v, w (12)

A "launch" is the entry point's three kernels (slab norms, per-tensor norms, apply).  Usage:
    python tools/optim_bench.py [--launches 400] [--warmup 20]        (one JSON line on stdout, prefixed OPTIM_BENCH)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def configs1_sizes():
    """Element counts of the trainable variables of configs[1], from the model itself (one tiny forward/backward builds them)."""
    import bench
    from boosted_detr_amd.engine import to_device
    args = type("A", (), dict(model="detr", fashionpedia=False, backbone="ResNet", image=640, image_w=0, layers=6, queries=100, learners=3, batch=2))()
    model = bench.build_model(args)
    h = bench.make_batch(2, 640, 640, 100, 82, seed=1)
    model.forward_backward({"image": to_device(h["image"]), "category": to_device(h["category"], torch.int32), "attribute": to_device(h["attribute"], torch.int32),
                            "bbox": to_device(h["bbox"]), "num_objects": to_device(h["num_objects"], torch.int32)})
    sizes = [v.value.numel() for v in model.trainable_variables]
    model.compile(optimizer=None)
    del model
    torch.cuda.empty_cache()
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="timed launches of EACH entry point (>= 200)")
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    assert a.launches >= 200
    from boosted_detr_amd.engine import Variable
    from boosted_detr_amd.training import SGD, AdamW
    sizes = configs1_sizes()
    n = int(sum(sizes))
    gen = torch.Generator(device="cuda").manual_seed(1)
    opts = {}
    for name, opt in (("sgd", SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1)), ("adamw", AdamW(1e-4, weight_decay=1e-3, clipnorm=0.1))):
        vs = []
        for i, s in enumerate(sizes):
            v = Variable(f"bench/t{i}", (s,))
            v.value = 0.05 * torch.randn(s, device="cuda", generator=gen)
            vs.append(v)
        opt.build(vs)
        opt.flat_grad.copy_(1e-3 * torch.randn(opt.flat_grad.numel(), device="cuda", generator=gen))
        opts[name] = opt
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(a.warmup):
        for opt in opts.values():
            opt.apply_gradients()
    torch.cuda.synchronize()
    events = {k: [] for k in opts}
    for _ in range(a.launches):
        for k, opt in opts.items():                       # alternating: both see the same clocks and the same neighbours
            opt.stage_lr()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt._launch(1.0, None, stream)
            e1.record()
            opt.iterations += 1
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {"parameters": n, "tensors": len(sizes), "slabs": opts["sgd"].nslabs, "launches_each": a.launches}
    for k, per in (("sgd", 24), ("adamw", 32)):
        us = np.asarray([e0.elapsed_time(e1) * 1e3 for e0, e1 in events[k]])
        assert all(bool(torch.isfinite(v.value).all()) for v in opts[k].vars[:4])
        out[k] = {"bytes_per_launch": per * n, "us_median": round(float(np.median(us)), 2), "us_mean": round(float(us.mean()), 2),
                  "us_min": round(float(us.min()), 2), "us_p90": round(float(np.percentile(us, 90)), 2),
                  "TBps_at_median": round(per * n / float(np.median(us)) * 1e-6, 3)}
    out["adamw_over_sgd_bytes_per_s"] = round(out["adamw"]["TBps_at_median"] / out["sgd"]["TBps_at_median"], 3)
    out["adamw_minus_sgd_us"] = round(out["adamw"]["us_median"] - out["sgd"]["us_median"], 2)
    print("OPTIM_BENCH " + json.dumps(out))


if __name__ == "__main__":
    main()
