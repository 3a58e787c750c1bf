"""Stream-schedule harness (plain torch; no kernel of its own).

In deterministic mode (kernels.set_deterministic(True)) a training step is a pure function of its inputs, so its result must not
depend on which of the step's two streams is ahead when a kernel runs.  The toy models of the suite are bound by host enqueue time:
the GPU is idle when each kernel arrives, both streams are serialised by the host, and a missing event or an operand freed too
early changes nothing.  This module forces the two extreme schedules with bounded spin kernels (torch.cuda._sleep):

  backlog    one sleep on the main stream right in front of train_step: the host enqueues the whole step while the GPU still sleeps,
             so every kernel of the step sits in a queue and is ordered by events alone.  A side task whose fork wait is missing
             runs during the sleep, on operands nobody has produced yet.
  late_side  the first wait of the side stream in each step is followed by one sleep ON the side stream: all side work starts after
             the main stream has finished the backward pass.  That exposes in-place overwrites of side-task operands, reuse of their
             memory and consumers that run ahead of the join.

and `run_leg` returns what a model computed under one of them, to be compared bit for bit with the stream-ordered step
(side stream off).  A leg whose schedule did not materialise (the effectiveness conditions of `Schedule.report`) is a failure.

Sleep lengths are sized in-process from the unperturbed leg of the same model (`sleep_lengths`); they are not pass bars.
"""
import contextlib
import sys
import time

import numpy as np

MAX_SLEEP_MS = 500.0          # no single sleep is longer, whatever was measured
SCHEDULES = ("reference", "unperturbed", "backlog", "late_side", "backlog+late_side")
MIN_EFFECTIVE_STEPS = 2       # non-exempt steps of a leg that must meet its effectiveness condition


# ---------------------------------------------------------------------------------------------------------------------------------
# arithmetic (tested on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def cycles_per_ms(cycles: int, elapsed_ms: float) -> float:
    """Spin-kernel cycles per millisecond from one timed call."""
    if not (cycles > 0 and elapsed_ms > 0.0):
        raise ValueError(f"calibration needs a positive measurement (cycles {cycles}, {elapsed_ms} ms)")
    return cycles / elapsed_ms


def sleep_cycles(ms: float, rate: float) -> int:
    """Cycles of one sleep of `ms` milliseconds at `rate` cycles / ms - never more than MAX_SLEEP_MS worth."""
    return int(min(max(float(ms), 0.0), MAX_SLEEP_MS) * rate)


def sleep_lengths(host_ms, gpu_ms) -> dict:
    """Sleeps of the two schedules from the unperturbed steps of the same model: backlog = 1.5 x the host wall time of train_step
    (no synchronisation), late_side = 1.5 x the step's GPU time between two events; the slowest measured step counts."""
    return {"backlog": min(1.5 * max(host_ms), MAX_SLEEP_MS), "late_side": min(1.5 * max(gpu_ms), MAX_SLEEP_MS)}


def differing(a: dict, b: dict) -> list:
    """Names whose arrays are not bit-identical (or exist on one side only), sorted."""
    bad = [k for k in a if k not in b or not np.array_equal(a[k], b[k])]
    return sorted(bad + [k for k in b if k not in a])


# ---------------------------------------------------------------------------------------------------------------------------------
# the device behind the schedules (a fake one in tests/test_schedule_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
class CudaBackend:
    _rate = [None]            # cycles / ms of torch.cuda._sleep, calibrated once per process

    def event(self, timing: bool = False):
        import torch
        return torch.cuda.Event(enable_timing=timing)

    def current_stream(self):
        import torch
        return torch.cuda.current_stream()

    def stream_ctx(self, stream):
        import torch
        return torch.cuda.stream(stream)

    def capturing(self) -> bool:
        import torch
        return torch.cuda.is_current_stream_capturing()

    def rate(self) -> float:
        if self._rate[0] is None:
            import torch
            torch.cuda._sleep(1000)              # (loads the kernel)
            torch.cuda.synchronize()
            cycles = 1_000_000
            for _ in range(4):                   # two timing events around ONE call; a longer call when the first was too short to time
                e0, e1 = self.event(True), self.event(True)
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 2.0:
                    break
                cycles *= 8
            self._rate[0] = cycles_per_ms(cycles, ms)
        return self._rate[0]

    def sleep(self, ms: float) -> bool:
        """One bounded spin kernel on the current stream; never on a capturing stream.  True when it was enqueued."""
        if self.capturing():
            return False
        import torch
        cycles = sleep_cycles(ms, self.rate())
        if cycles > 0:
            torch.cuda._sleep(cycles)
        return cycles > 0


class LateSide:
    """Mix-in in front of a stream class: the first `wait_event` of each step is followed by one sleep on the stream itself, and
    `record_event` - what `main.wait_stream(side)` calls at the join - re-arms "first of the step".  Both keep timing events: the
    moment the side stream's first task of the step may start, and the moment the main stream reaches the join."""
    _late = None

    def arm(self, backend, ms: float) -> None:
        self._late = {"backend": backend, "ms": float(ms), "first": True, "step": None, "starts": {}, "joins": {}}

    def begin_step(self, step: int) -> None:
        self._late["step"], self._late["first"] = step, True

    def wait_event(self, event) -> None:
        super().wait_event(event)
        s = self._late
        if s is None or not s["first"] or s["backend"].capturing():
            return
        s["first"] = False
        b = s["backend"]
        with b.stream_ctx(self):
            slept = b.sleep(s["ms"])
            start = b.event(True)
            start.record(self)
        s["starts"][s["step"]] = (start, slept)

    def record_event(self, event=None):
        s = self._late
        if s is not None and not s["backend"].capturing():
            b = s["backend"]
            mark = b.event(True)
            mark.record(b.current_stream())      # the main stream, just before it waits for the side stream
            s["joins"][s["step"]] = mark
            s["first"] = True
        return super().record_event(event)


def late_side_stream(real):
    """The real side stream's HIP stream behind a LateSide object (torch.cuda.ExternalStream on the same handle: not a new stream)."""
    import torch

    class LateSideStream(LateSide, torch.cuda.ExternalStream):
        pass

    return LateSideStream(real.cuda_stream, device=real.device)


class Schedule:
    """One leg's schedule: installs itself, perturbs every step, and reports whether the schedule really took place."""

    def __init__(self, kind: str, sizes=None, backend=None, wrap=late_side_stream):
        if kind not in SCHEDULES:
            raise ValueError(kind)
        self.kind, self.backend, self.wrap = kind, backend or CudaBackend(), wrap
        self.backlog, self.late = "backlog" in kind, "late_side" in kind
        if (self.backlog or self.late) and sizes is None:
            raise ValueError(f"schedule '{kind}' needs sleep lengths (sleep_lengths of the unperturbed leg)")
        self.sizes = dict(sizes or {})
        self.side = None
        self.steps = []

    @contextlib.contextmanager
    def installed(self, engine):
        """The late side stream stands in as engine._SIDE["stream"] for the duration (on_side_stream and SegmentedCapture.replay(side)
        both take the stream from there)."""
        if not self.late:
            yield self
            return
        real = engine.side_stream()
        if real is None:
            raise RuntimeError("late_side needs the side stream (engine.set_side_stream_enabled(True))")
        self.side = self.wrap(real)
        self.side.arm(self.backend, self.sizes["late_side"])
        engine._SIDE["stream"] = self.side
        try:
            yield self
        finally:
            engine._SIDE["stream"] = real

    def before_step(self, step: int) -> None:
        b = self.backend
        if self.side is not None:
            self.side.begin_step(step)
        slept = b.sleep(self.sizes["backlog"]) if self.backlog else False
        begin = b.event(True)
        begin.record()                           # right behind the sleep
        self.steps.append({"step": step, "begin": begin, "slept": slept, "t0": time.perf_counter()})

    def after_step(self, exempt: bool = False) -> None:
        """Directly behind train_step's return.  exempt: the model itself synchronised in this step (capture, guard redo)."""
        s = self.steps[-1]
        s["host_ms"] = (time.perf_counter() - s.pop("t0")) * 1e3
        s["pending"] = not s["begin"].query()    # the GPU has not even finished the sleep: the whole step sits in the queues
        s["end"] = self.backend.event(True)
        s["end"].record()
        s["exempt"] = bool(exempt)

    def report(self) -> dict:
        """After the device has been synchronised: per-step times and what failed to materialise ("problems", empty when all is well)."""
        out = {"kind": self.kind, "sleep_ms": {k: round(v, 3) for k, v in self.sizes.items()}, "host_ms": [], "gpu_ms": [], "exempt": [],
               "backlog_pending": [], "side_start_after_join_ms": [], "problems": []}
        starts = self.side._late["starts"] if self.side is not None else {}
        joins = self.side._late["joins"] if self.side is not None else {}
        for s in self.steps:
            out["host_ms"].append(round(s["host_ms"], 3))
            out["gpu_ms"].append(round(s["begin"].elapsed_time(s["end"]), 3))
            if s["exempt"]:
                out["exempt"].append(s["step"])
            if self.backlog:
                out["backlog_pending"].append(bool(s["pending"] and s["slept"]))
            if self.late:
                lag = None
                if s["step"] in starts and s["step"] in joins and starts[s["step"]][1]:
                    lag = round(joins[s["step"]].elapsed_time(starts[s["step"]][0]), 3)      # start - join
                out["side_start_after_join_ms"].append(lag)
        live = [i for i, s in enumerate(self.steps) if not s["exempt"]]
        if self.backlog:
            ok = [i for i in live if out["backlog_pending"][i]]
            if len(ok) < len(live) or len(ok) < MIN_EFFECTIVE_STEPS:
                out["problems"].append(f"backlog did not materialise: the sleep was still pending at train_step's return in steps "
                                       f"{[self.steps[i]['step'] for i in ok]} of the non-exempt {[self.steps[i]['step'] for i in live]}")
        if self.late:
            lags = out["side_start_after_join_ms"]
            ok = [i for i in live if lags[i] is not None and lags[i] >= 0.0]
            if len(ok) < len(live) or len(ok) < MIN_EFFECTIVE_STEPS:
                out["problems"].append(f"late_side did not materialise: side start minus join per step {lags} ms (None: no fork wait or no join "
                                       f"seen), non-exempt steps {[self.steps[i]['step'] for i in live]}")
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# path counters
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def count_paths():
    """Counts the in-place paths of the backward pass by wrapping their entry points for the duration: the masked-accumulate and the
    accumulating 1x1 backward-data epilogues, the lazy-skip branch of ops._p16_bn_backward (the incoming gradient handed on as the skip
    gradient), and relu_mask_apply_ / axpy_ by caller (engine.py: the Tape and materialise; elsewhere: gradient sinks)."""
    from boosted_detr_amd import engine, kernels as K, ops, panoptic_neck
    counts = {"masked_accum": 0, "bwd_data_accumulate": 0, "lazy_skip": 0, "tape_relu_mask_apply": 0, "tape_axpy": 0, "sink_axpy": 0, "side_tasks": 0}
    real = {"masked": K.p16_conv2d_bwd_data_masked_accum, "bwd": K.p16_conv2d_bwd_data, "bn": ops._p16_bn_backward,
            "mask": K.relu_mask_apply_, "axpy": K.axpy_, "task": ops.side_task}

    def from_engine() -> bool:
        return sys._getframe(2).f_code.co_filename.endswith("engine.py")

    def masked(*a, **kw):
        counts["masked_accum"] += 1
        return real["masked"](*a, **kw)

    def bwd(dy, wt, g, dx=None, accumulate=False):
        counts["bwd_data_accumulate"] += bool(accumulate)
        return real["bwd"](dy, wt, g, dx=dx, accumulate=accumulate)

    def bn(*a, **kw):
        dyb, dres = real["bn"](*a, **kw)
        counts["lazy_skip"] += dres is not None and engine.info(dres).lazy_mask is not None
        return dyb, dres

    def mask(x, m):
        counts["tape_relu_mask_apply"] += from_engine()
        return real["mask"](x, m)

    def axpy(alpha, x, y):
        counts["tape_axpy" if from_engine() else "sink_axpy"] += 1
        return real["axpy"](alpha, x, y)

    def task(fn, *keep):
        counts["side_tasks"] += 1
        return real["task"](fn, *keep)

    K.p16_conv2d_bwd_data_masked_accum, K.p16_conv2d_bwd_data, ops._p16_bn_backward = masked, bwd, bn
    K.relu_mask_apply_, K.axpy_, ops.side_task, panoptic_neck.side_task = mask, axpy, task, task
    try:
        yield counts
    finally:
        K.p16_conv2d_bwd_data_masked_accum, K.p16_conv2d_bwd_data, ops._p16_bn_backward = real["masked"], real["bwd"], real["bn"]
        K.relu_mask_apply_, K.axpy_, ops.side_task, panoptic_neck.side_task = real["mask"], real["axpy"], real["task"], real["task"]


# ---------------------------------------------------------------------------------------------------------------------------------
# legs
# ---------------------------------------------------------------------------------------------------------------------------------
def run_leg(build, batches, steps: int, schedule: str, sizes=None, each_step=None):
    """`steps` train_steps of build() under `schedule`: (losses, weights dict, path counters).  "reference" runs with the side stream
    off (one stream: the order of the program); every other schedule with it on.  No host read between the steps; the per-step loss
    vectors are cloned on the device and reduced afterwards.  each_step(model, i) runs in front of step i.  counters["schedule"] is
    Schedule.report()."""
    import torch
    from boosted_detr_amd import engine
    was_on = engine._SIDE["enabled"]
    engine.set_side_stream_enabled(schedule != "reference")
    try:
        model = build()
        torch.cuda.synchronize()
        sched = Schedule(schedule, sizes)
        kept = []
        with sched.installed(engine), count_paths() as counts:
            for i in range(steps):
                if each_step is not None:
                    each_step(model, i)
                # steps in which the model itself waits for the device are exempt from the effectiveness conditions: a capture
                # (torch.cuda.graph synchronises on entry), a guard redo, and the optimizer (re)building its flat buffers (pageable
                # host-to-device copies of its tables: the first step, the step behind a change of the trainable set)
                state = lambda: (len(model._graphs), model.guard.redos, id(getattr(model.optimizer, "flat_grad", None)))
                before = state()
                sched.before_step(i)
                logs = model.train_step(batches[i % len(batches)])
                sched.after_step(exempt=state() != before)
                kept.append({k: [t.detach().clone() for t in v] for k, v in logs.items()})
            model.guard_flush()
            torch.cuda.synchronize()
        counters = dict(counts, schedule=sched.report(), graphs=len(model._graphs), range_redos=model.guard.redos)
        losses = [model.logs_to_host(l)["loss"] for l in kept]
        return losses, model.get_weights_dict(), counters
    finally:
        engine.set_side_stream_enabled(was_on)


def leg_problems(ref, leg, name: str) -> list:
    """Everything wrong with one leg against the reference leg: a loss or a weight that is not bit-identical (named), a schedule that
    did not materialise."""
    problems = []
    bad_steps = [i for i, (a, b) in enumerate(zip(ref[0], leg[0])) if not a == b]
    if len(ref[0]) != len(leg[0]) or bad_steps:
        problems.append(f"{name}: losses differ from the stream-ordered step at steps {bad_steps}: {leg[0]} vs {ref[0]}")
    bad = differing(ref[1], leg[1])
    if bad:
        problems.append(f"{name}: {len(bad)} of {len(ref[1])} weights differ from the stream-ordered step, first {bad[:4]}")
    problems += [f"{name}: {p}" for p in leg[2]["schedule"]["problems"]]
    return problems


def run_all_legs(build, batches, steps: int, build_reference=None, each_step=None):
    """The reference leg and the four schedules of one model; returns ({schedule: leg}, problems).  The sleeps of the three
    perturbed legs come from the unperturbed one's steps (steps in which the model synchronised - a capture - left out)."""
    legs = {"reference": run_leg(build_reference or build, batches, steps, "reference", each_step=each_step)}
    sizes, problems = None, []
    for kind in SCHEDULES[1:]:
        legs[kind] = run_leg(build, batches, steps, kind, sizes, each_step=each_step)
        rep = legs[kind][2]["schedule"]
        if kind == "unperturbed":
            live = [i for i in range(steps) if i not in rep["exempt"]]
            sizes = sleep_lengths([rep["host_ms"][i] for i in live], [rep["gpu_ms"][i] for i in live])
        found = leg_problems(legs["reference"], legs[kind], kind)
        problems += found
        show = {k: v for k, v in legs[kind][2].items() if k != "schedule"}
        print(f"[schedule] {kind}: {'FAIL' if found else 'ok'} sleeps {rep['sleep_ms']} host_ms {rep['host_ms']} gpu_ms {rep['gpu_ms']} exempt {rep['exempt']} "
              f"backlog_pending {rep['backlog_pending']} side_start_after_join_ms {rep['side_start_after_join_ms']} counters {show}")
    return legs, problems
