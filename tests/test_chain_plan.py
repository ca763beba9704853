"""The host logic of chained single launches, without a GPU:

* ``wgrt_debug_chain_plan`` (the rule ``wgrt_chain_step`` follows): which stream a step goes to, what it waits
  for and publishes, when a segment opens, closes, or a step runs as a plain launch;
* ``distributed.run_steps`` issues separate launches as a chain exactly when the tracer offers one,
  ``per_call == 1``, ``steps > 1`` and there is no hook, and always closes it."""
import pytest

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import CHAIN_SERIAL_MAX, chain_plan
from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import GidMap, run_steps

FLAGS = [_lib.CHAIN_LEARNS, _lib.CHAIN_VARIANT1, _lib.CHAIN_SINGLE, _lib.CHAIN_FUSED, _lib.CHAIN_DEBUG,
         _lib.CHAIN_CAPTURE, _lib.CHAIN_FULL]


def _walk(steps, serial=0, flags=lambda k: 0):
    """The plans of ``steps`` consecutive steps of one chain."""
    seg, out = -1, []
    for k in range(steps):
        p = chain_plan(seg, serial, flags(k))
        seg, serial = p["in_segment_after"], p["serial_after"]
        out.append(p)
    return out


def test_steps_alternate_and_hand_over_in_order():
    """The first step seeds the segment (serial 1) on the caller's stream; step k goes to side k % 2, takes its
    states from the tag the step before published and publishes the next serial; no step but the first costs a
    seed or a join."""
    plans = _walk(6)
    assert [p["side"] for p in plans] == [0, 1, 0, 1, 0, 1]
    assert [p["seed"] for p in plans] == [1, 0, 0, 0, 0, 0]
    assert all(p["chained"] and not p["join"] and not p["clear"] for p in plans)
    assert [p["wait_serial"] for p in plans] == [1, 2, 3, 4, 5, 6]
    assert [p["publish_serial"] for p in plans] == [2, 3, 4, 5, 6, 7]
    assert plans[-1]["serial_after"] == 7 and plans[-1]["in_segment_after"] == 6


def test_a_later_chain_continues_the_serial():
    """Stale granules never match: a new segment's serials lie above everything an earlier one published."""
    first = _walk(3)
    second = _walk(2, serial=first[-1]["serial_after"])
    assert second[0]["seed"] == 1 and second[0]["side"] == 0
    assert second[0]["wait_serial"] > first[-1]["publish_serial"]


@pytest.mark.parametrize("flag", FLAGS)
def test_every_flag_makes_a_plain_launch_behind_a_join(flag):
    plans = _walk(5, flags=lambda k: flag if k == 2 else 0)
    assert [p["chained"] for p in plans] == [1, 1, 0, 1, 1]
    assert plans[2]["join"] == 1 and plans[2]["side"] == 0 and plans[2]["seed"] == 0
    assert plans[2]["in_segment_after"] == -1 and plans[2]["serial_after"] == plans[1]["serial_after"]
    # the step after it opens a new segment on the caller's stream
    assert plans[3]["seed"] == 1 and plans[3]["join"] == 0 and plans[3]["side"] == 0
    assert plans[4]["side"] == 1
    # with no segment open there is nothing to join
    assert chain_plan(-1, 7, flag)["join"] == 0


def test_serial_wrap_closes_the_segment_and_clears():
    """The tag serial runs out inside a chain: join, clear, reseed from serial 1; chains of any length work."""
    plans = _walk(4, serial=CHAIN_SERIAL_MAX - 2)
    assert plans[0]["seed"] == 1 and plans[0]["clear"] == 0 and plans[0]["publish_serial"] == CHAIN_SERIAL_MAX
    assert plans[1]["join"] == 1 and plans[1]["clear"] == 1 and plans[1]["seed"] == 1
    assert plans[1]["side"] == 0 and plans[1]["wait_serial"] == 1 and plans[1]["publish_serial"] == 2
    assert plans[2]["side"] == 1 and not plans[2]["join"] and plans[3]["side"] == 0
    # a chain that begins with too little room for a seed and a step clears first
    p = chain_plan(-1, CHAIN_SERIAL_MAX - 1)
    assert p["clear"] == 1 and p["join"] == 0 and p["publish_serial"] == 2


def test_bad_arguments_are_refused():
    with pytest.raises(_lib.WgrtError):
        chain_plan(-2, 0)
    with pytest.raises(_lib.WgrtError):
        chain_plan(0, CHAIN_SERIAL_MAX + 1)


class _FakeTracer:
    """A tracer that records its calls and, with ``offer``, offers a chain that records its own."""

    def __init__(self, offer=True):
        self.calls, self.chains = [], []
        if offer:
            self.chain = self._chain

    def __call__(self, rays, rng, eb, gid, num_iter=1):
        self.calls.append(num_iter)

    def _chain(self, rays, rng, eb, gid):
        tracer = self

        class Chain:
            steps, closed, raised = 0, False, None

            def __enter__(self):
                return self

            def step(self):
                self.steps += 1
                if self.steps == tracer.fail_at:
                    raise RuntimeError("step failed")

            def __exit__(self, et, ev, tb):
                self.closed, self.raised = True, et
                return False
        ch = Chain()
        self.chains.append(ch)
        return ch
    fail_at = 0


GID = GidMap([0], 8)


def test_run_steps_uses_the_chain_for_separate_launches():
    t = _FakeTracer()
    assert run_steps(t, None, None, None, GID, 5, 1) == [1] * 5
    assert t.calls == [] and len(t.chains) == 1 and t.chains[0].steps == 5 and t.chains[0].closed


@pytest.mark.parametrize("steps,per_call,hook", [(1, 1, False), (5, 0, False), (5, 2, False), (5, 1, True), (0, 1, False)])
def test_run_steps_stays_serial_otherwise(steps, per_call, hook):
    t = _FakeTracer()
    seen = []
    calls = run_steps(t, None, None, None, GID, steps, per_call, (lambda j, what: seen.append((j, what))) if hook else None)
    assert t.chains == [] and t.calls == calls and sum(calls) == steps
    if hook:
        assert seen == [(j, w) for j in range(steps) for w in ("start", "end")]


def test_run_steps_without_a_chain_attribute_runs_as_before():
    t = _FakeTracer(offer=False)
    assert run_steps(t, None, None, None, GID, 4, 1) == [1] * 4 and t.calls == [1] * 4


def test_run_steps_closes_the_chain_on_an_exception():
    t = _FakeTracer()
    t.fail_at = 2
    with pytest.raises(RuntimeError, match="step failed"):
        run_steps(t, None, None, None, GID, 4, 1)
    assert t.chains[0].closed and t.chains[0].raised is RuntimeError and t.chains[0].steps == 2
