"""The hand-scheduled critic iterations ask the layers below them for exactly the recorded launches: the same kernel
wrappers with the same operands (by storage, offset, shape and strides) in the same order, the same ATen operators in
between, `on_grads` at the same points - and, on the GPU, on the same streams with the same fork, join and
record_stream edges. The traces were recorded from the commit before critic_step.py was split into a schedule and two
branch objects (tests/critic_trace.py says how, and when to record again)."""
import pytest

from tests import critic_trace as CT


def _same(name):
    got, want = CT.trace(name), CT.recorded(name)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: entry %d differs\n  recorded: %s\n  now:      %s" % (name, i, w, g)
    assert len(got) == len(want), "%s: %d entries, recorded %d; the first one without a partner: %s" % (
        name, len(got), len(want), max(got, want, key=len)[min(len(got), len(want))])


@pytest.mark.parametrize("name", sorted(CT.CPU_CASES))
def test_launch_trace_equals_the_recorded_one(name):
    _same(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CT.GPU_CASES))
def test_launch_trace_with_streams_equals_the_recorded_one(name):
    _same(name)
