#!/usr/bin/env python3
"""Cost of `valid_region` in the training step at BASELINE.json configs[1] (batch 16, 640 x 640, 6 + 6 layers, 100 queries).

    python tools/padding_mask_bench.py [--out FILE] [--steps 60]
        the training step, enqueued eagerly and replayed from its captured graphs, with (a) no key, (b) a full-image key, (c) regions
        drawn as pipeline.Augmentations.draw draws them (eight draws, another one every step) - all in THIS process, interleaved
        window by window (windows of 10 steps, a device-synchronised host clock around each).  No figure is a pass mark.

    python tools/padding_mask_bench.py --no-key-only --label NAME [--package-root DIR]
        one process's two series of the step WITHOUT the key, for alternating-process comparisons of two trees: the package is
        imported from DIR (a checkout of another commit with its library built) instead of this tree.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/padding_mask_bench.py --kernel-run
        twelve eager steps with drawn regions and nothing else, for the profiler's own kernel times (token_key_mask_kernel and the
        masked attention kernels; reduce with tools/kstats.py).

A measurement path that finds no GPU fails."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, IMAGE, LAYERS, QUERIES, MAX_OBJECTS, CLASSES = 16, 640, 6, 100, 100, 82
WINDOW = 10


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--no-key-only", action="store_true")
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--package-root", default=HERE)
    return ap.parse_args()


ARGS = parse()
sys.path.insert(0, os.path.abspath(ARGS.package_root))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import boosted_detr_amd  # noqa: E402

boosted_detr_amd.enable_graph_replay()          # before HIP initialises (see the package's __init__)


def make_batch(seed):
    """bench.py's synthetic inputs, restated."""
    rng = np.random.Generator(np.random.PCG64(seed))
    image = rng.random((B, IMAGE, IMAGE, 3), dtype=np.float32)
    num_objects = np.clip(1 + rng.poisson(6.3, size=B), 1, 93).astype(np.int32)
    category = np.zeros((B, MAX_OBJECTS), np.int32)
    attribute = np.zeros((B, MAX_OBJECTS, 3), np.int32)
    bbox = np.full((B, MAX_OBJECTS, 4), -10.0, np.float32)
    for b in range(B):
        n = int(num_objects[b])
        category[b, :n] = rng.integers(2, CLASSES, size=n)
        bbox[b, :n, 0:2] = rng.uniform(0.0, 0.6, size=(n, 2))
        bbox[b, :n, 2:4] = rng.uniform(0.05, 0.4, size=(n, 2))
    return {"image": image, "category": category, "attribute": attribute, "bbox": bbox, "num_objects": num_objects}


def build_model():
    from boosted_detr_amd import parameters
    from boosted_detr_amd.model import DETR
    from boosted_detr_amd.training import SGD, CosineDecayRestarts
    model = DETR(num_object_preds=QUERIES, image_size=(IMAGE, IMAGE), num_encoder_blocks=LAYERS, num_encoder_heads=8, encoder_dim=256,
                 num_decoder_blocks=LAYERS, num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32,
                 vocab_dict=parameters.COCO_VOCAB, attribute_weight=0.0)
    model.compile(optimizer=SGD(CosineDecayRestarts(1e-3, 4000, m_mul=0.95, alpha=0.1), momentum=0.9, nesterov=True, clipnorm=0.1))
    return model


def drawn_regions(n):
    from boosted_detr_amd.pipeline import Augmentations
    aug = Augmentations(seed=5, jpeg_quality=False)
    out = []
    for _ in range(n):
        p = aug.draw(B, IMAGE, IMAGE)
        out.append(np.stack([p["off_h"], p["off_w"], p["new_h"], p["new_w"]], axis=-1).astype(np.int32))
    return out


class Variant:
    def __init__(self, name, batches, graph):
        self.name, self.batches, self.graph, self.i, self.ms = name, batches, graph, 0, []

    def step(self, model):
        model.use_graph = self.graph
        model.train_step(self.batches[self.i % len(self.batches)])
        self.i += 1

    def window(self, model, n=WINDOW):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step(model)
        torch.cuda.synchronize()
        self.ms.append((time.perf_counter() - t0) / n * 1e3)

    def line(self):
        return "%-34s %7.3f ms / step   (windows %.3f - %.3f, %d steps)" % (self.name, statistics.median(self.ms), min(self.ms), max(self.ms),
                                                                           WINDOW * len(self.ms))


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing measured")
    from boosted_detr_amd.engine import to_device
    host = make_batch(1234)
    base = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
            "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32)}
    model = build_model()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    kinds = [("no key", [base])]
    if not a.no_key_only:
        full = to_device(np.array([[0, 0, IMAGE, IMAGE]] * B, np.int32), torch.int32)
        draws = drawn_regions(8)
        kinds += [("full-image key", [dict(base, valid_region=full)]),
                  ("drawn regions", [dict(base, valid_region=to_device(g, torch.int32)) for g in draws])]
    if a.kernel_run:
        v = Variant("drawn regions, eager", kinds[2][1], False)
        for _ in range(12):
            v.step(model)
        torch.cuda.synchronize()
        return
    variants = [Variant("%s, %s" % (name, "replayed" if graph else "eager"), batches, graph) for graph in (False, True) for name, batches in kinds]
    for v in variants:                      # set-up: build-by-first-call, allocator warm-up, the capture (third step on a signature), warm-up
        for _ in range(6):
            v.step(model)
        torch.cuda.synchronize()
        if v.graph and not model._graphs:
            raise SystemExit("the step was not captured (graph replay refused): nothing measured")
    for _ in range(max(1, -(-a.steps // WINDOW))):
        for v in variants:
            v.window(model)
    model.guard_flush()
    if a.no_key_only:
        say("  %-10s %s   |   %s" % (a.label, variants[0].line(), variants[1].line()))
    else:
        say("training step with `valid_region` - tools/padding_mask_bench.py; device: %s" % torch.cuda.get_device_name(0))
        say("configs[1]: batch %d, %d x %d, %d + %d layers, %d queries, 'split' policy; one model, the variants interleaved window by window"
            % (B, IMAGE, IMAGE, LAYERS, LAYERS, QUERIES))
        say("(windows of %d steps, device-synchronised host clock); median over the windows (min - max).  No figure is a pass mark." % WINDOW)
        if len(kinds) > 2:
            from boosted_detr_amd import kernels as K
            keep = [K.token_keep_host(g, IMAGE, IMAGE, 20, 20).mean() for g in draws]
            say("drawn regions: eight draws of Augmentations.draw, kept tokens per draw %s of 400 per image on average"
                % ", ".join("%.0f" % (400 * k) for k in keep))
        for v in variants:
            say("  " + v.line())
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
