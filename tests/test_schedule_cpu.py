"""Host side of the stream-schedule harness (tests/_schedule.py) without a GPU: the bit-exact comparison names what differs, the sleep
arithmetic and its cap, and - on logged fake streams with a logical clock - a schedule that did not materialise makes its leg fail."""
import types

import numpy as np
import pytest

import _schedule as S


# ---------------------------------------------------------------- comparison
def _leg(losses, weights, problems=()):
    return (list(losses), weights, {"schedule": {"problems": list(problems)}})


def test_a_one_bit_difference_in_one_weight_is_reported_by_name():
    rng = np.random.default_rng(7)
    ref = {f"Layer_{i}/kernel": rng.standard_normal((3, 5)).astype(np.float32) for i in range(6)}
    got = {k: v.copy() for k, v in ref.items()}
    assert S.differing(ref, got) == [] and S.leg_problems(_leg([1.5, 2.5], ref), _leg([1.5, 2.5], got), "late_side") == []
    name = "Layer_4/kernel"
    got[name].view(np.uint32)[int(rng.integers(3)), int(rng.integers(5))] ^= 1          # the lowest mantissa bit of one element
    assert np.allclose(ref[name], got[name], rtol=1e-6, atol=0)                           # ... which a tolerance would not see
    assert S.differing(ref, got) == [name]
    problems = S.leg_problems(_leg([1.5, 2.5], ref), _leg([1.5, 2.5], got), "late_side")
    assert len(problems) == 1 and name in problems[0] and problems[0].startswith("late_side:") and "1 of 6 weights" in problems[0]


def test_losses_compare_with_equality_and_missing_weights_count():
    w = {"a": np.zeros(2, np.float32)}
    assert S.leg_problems(_leg([1.0, 2.0], w), _leg([1.0, np.nextafter(2.0, 3.0)], w), "backlog")[0].count("steps [1]") == 1
    assert S.leg_problems(_leg([1.0], w), _leg([float("nan")], w), "backlog")              # NaN never equals the reference
    assert S.differing(w, {}) == ["a"] and S.differing({}, w) == ["a"]
    assert S.differing({"a": np.float32([0.0, 0.0])}, {"a": np.float32([0.0, -0.0])}) == []      # np.array_equal, as test_training_gpu._same_weights
    assert S.leg_problems(_leg([1.0], w), _leg([1.0], w, ["backlog did not materialise"]), "backlog") == ["backlog: backlog did not materialise"]


# ---------------------------------------------------------------- arithmetic
def test_calibration_arithmetic_and_the_500_ms_cap():
    assert S.MAX_SLEEP_MS == 500.0
    rate = S.cycles_per_ms(8_000_000, 3.2)
    assert rate == 2_500_000.0
    assert S.sleep_cycles(2.0, rate) == 5_000_000
    assert S.sleep_cycles(500.0, rate) == S.sleep_cycles(1e9, rate) == S.sleep_cycles(float("inf"), rate) == 1_250_000_000
    assert S.sleep_cycles(0.0, rate) == S.sleep_cycles(-3.0, rate) == 0
    for bad in ((0, 1.0), (1000, 0.0), (1000, -1.0), (1000, float("nan"))):
        with pytest.raises(ValueError):
            S.cycles_per_ms(*bad)
    assert S.sleep_lengths([40.0, 60.0, 50.0], [3.0, 70.0]) == {"backlog": 90.0, "late_side": 105.0}       # 1.5 x the slowest step
    assert S.sleep_lengths([400.0], [1000.0]) == {"backlog": 500.0, "late_side": 500.0}


# ---------------------------------------------------------------- fake streams with a logical clock
class World:
    """Two in-order queues with a clock each (ms); an event carries the clock of the stream it was recorded on; a wait advances the
    waiting stream to it.  `host` is the wall clock: an event has happened (query) once the host clock has passed it."""

    def __init__(self, capturing=False, sleep_works=True):
        self.log, self.host, self.is_capturing, self.sleep_works = [], 0.0, capturing, sleep_works
        world = self

        class Stream:
            def __init__(self, name): self.name, self.clock = name, 0.0
            def wait_event(self, ev): world.log.append(("wait_event", self.name, ev.on)); self.clock = max(self.clock, ev.t)
            def record_event(self, event=None):
                event = event or Event()
                event.record(self)
                return event
            def wait_stream(self, other): self.wait_event(other.record_event())
            def work(self, ms): self.clock = max(self.clock, world.host) + ms

        class Event:
            def __init__(self, enable_timing=False): self.t, self.on = None, None
            def record(self, st=None): st = st or world.cur; self.t, self.on = max(st.clock, world.host), st.name; world.log.append(("record", st.name))
            def query(self): return self.t <= world.host
            def elapsed_time(self, other): return other.t - self.t

        class Ctx:
            def __init__(self, st): self.st = st
            def __enter__(self): self.prev, world.cur = world.cur, self.st
            def __exit__(self, *a): world.cur = self.prev

        self.Stream, self.Event = Stream, Event
        self.main, self.side_real = Stream("main"), Stream("side")
        self.cur = self.main
        self.backend = types.SimpleNamespace(event=lambda timing=False: Event(timing), current_stream=lambda: world.cur, stream_ctx=Ctx,
                                             capturing=lambda: world.is_capturing, sleep=self.sleep)
        self.engine = types.SimpleNamespace(_SIDE={"stream": self.side_real}, side_stream=lambda: self.engine._SIDE["stream"])

    def sleep(self, ms):
        if self.is_capturing:
            return False
        self.log.append(("sleep", self.cur.name, ms))
        if self.sleep_works:
            self.cur.work(ms)
        return True

    def wrap(self, real):
        class Late(S.LateSide, self.Stream):
            pass
        late = Late("side")
        late.clock = real.clock
        return late

    def train_step(self, host_ms=10.0, fwd=2.0, bwd=3.0, tasks=3, join=True, synchronise=False):
        """The product's structure: forward on main, `tasks` forks (event on main, side waits, side works), the join, the optimizer.
        The host needs host_ms for all of it; synchronise: the model waited for the device inside the step."""
        side = self.engine._SIDE["stream"]
        self.main.work(fwd)
        for _ in range(tasks):
            self.main.work(bwd / tasks)
            ev = self.Event()
            ev.record(self.main)
            side.wait_event(ev)
            side.work(1.0)
        if join:
            self.main.wait_stream(side)
        self.main.work(0.5)
        self.host += host_ms
        if synchronise:
            self.host = max(self.host, self.main.clock, side.clock)


def _run(world, kind, sizes, steps=3, exempt=(), **step_kw):
    sched = S.Schedule(kind, sizes, backend=world.backend, wrap=world.wrap)
    with sched.installed(world.engine):
        for i in range(steps):
            sched.before_step(i)
            world.train_step(synchronise=i in exempt, **step_kw)
            sched.after_step(exempt=i in exempt)
    assert world.engine._SIDE["stream"] is world.side_real           # restored
    world.host = 1e9                                                 # "synchronised"
    return sched.report()


SIZES = {"backlog": 15.0, "late_side": 15.0}


def test_schedules_that_materialise_pass_and_touch_the_streams_as_specified():
    w = World()
    rep = _run(w, "backlog+late_side", SIZES)
    assert rep["problems"] == [] and rep["backlog_pending"] == [True] * 3 and all(l >= 0 for l in rep["side_start_after_join_ms"])
    sleeps = [e for e in w.log if e[0] == "sleep"]
    assert sleeps == [("sleep", "main", 15.0), ("sleep", "side", 15.0)] * 3          # one per stream and step: the first side wait only
    for i, e in enumerate(w.log):
        if e == ("sleep", "side", 15.0):
            assert w.log[i - 1][:2] == ("wait_event", "side")                           # the side sleep FOLLOWS the fork wait
    assert _run(World(), "unperturbed", None)["problems"] == [] and _run(World(), "reference", None)["problems"] == []
    with pytest.raises(ValueError):
        S.Schedule("backlog", None, backend=w.backend)


def test_an_unmet_backlog_condition_fails_the_leg():
    rep = _run(World(), "backlog", {"backlog": 4.0, "late_side": 0.0})                # shorter than the host's 10 ms of enqueueing
    assert rep["backlog_pending"] == [False, False, False] and len(rep["problems"]) == 1 and "backlog did not materialise" in rep["problems"][0]
    rep = _run(World(sleep_works=False), "backlog", SIZES)                             # a sleep primitive that returns at once
    assert rep["problems"]
    w = {"a": np.zeros(1, np.float32)}
    assert S.leg_problems(([1.0], w, {}), ([1.0], w, {"schedule": rep}), "backlog")    # ... is a failure of the leg, identical values or not


def test_an_unmet_late_side_condition_fails_the_leg():
    rep = _run(World(), "late_side", {"backlog": 0.0, "late_side": 1.0})              # side work starts long before main reaches the join
    assert all(l < 0 for l in rep["side_start_after_join_ms"]) and "late_side did not materialise" in rep["problems"][0]
    rep = _run(World(), "late_side", SIZES, join=False)                                # no join seen: nothing to compare against
    assert rep["side_start_after_join_ms"] == [None] * 3 and rep["problems"]
    rep = _run(World(), "late_side", SIZES, tasks=0)                                   # no fork wait: the side stream never slept
    assert rep["problems"]


def test_no_sleep_enters_a_capturing_stream():
    w = World(capturing=True)
    rep = _run(w, "backlog+late_side", SIZES)
    assert not [e for e in w.log if e[0] == "sleep"] and len(rep["problems"]) == 2      # nothing enqueued, and the leg says so
    import inspect
    assert "capturing()" in inspect.getsource(S.CudaBackend.sleep)


def test_exempt_steps_are_left_out_but_two_effective_steps_remain_mandatory():
    # step 1 synchronises inside the model (a capture): its backlog is gone, the others' is not
    rep = _run(World(), "backlog", SIZES, steps=3, exempt=(1,))
    assert rep["backlog_pending"] == [True, False, True] and rep["exempt"] == [1] and rep["problems"] == []
    rep = _run(World(), "backlog", SIZES, steps=2, exempt=(1,))                        # one effective step is not enough
    assert rep["problems"]
    rep = _run(World(), "late_side", SIZES, steps=2, exempt=(0,))
    assert rep["problems"]
