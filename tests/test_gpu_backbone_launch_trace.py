"""GPU: the backbones and the neck hand the library what tests/golden/backbone_launch_traces.json recorded -- every ``lib.call`` of three forwards in plan mode
(weight packing and the eager warm-up, the recording, the replay), entry by entry and argument by argument: dtype codes, epilogues, tile variants, M / N / K,
leading dimensions, window strides and counts, tensor dtypes and shapes (addresses as "ptr"), and in the recording every launch's lane handle and every
``toc3d_plan_wait`` edge.  Cases, normalisation and the recorder are tools/gen_backbone_launch_traces.py's, which wrote the file; a change that alters the
launches on purpose regenerates it."""
import pytest

from tools.gen_backbone_launch_traces import FORWARDS, cases, load, trace

pytestmark = pytest.mark.gpu
CASES = cases()
GOLDEN = load()
LANE0 = 0x70c3d000


def test_the_recorded_cases_are_the_generators():
    assert sorted(GOLDEN) == sorted(CASES)
    for name, (first, record, replay) in GOLDEN.items():
        assert len(first) > len(record) > len(replay) > 0, f"{name}: the pack launches on top of the first forward, one toc3d_plan_run in the third"
        assert sum(c[0] == "toc3d_plan_run" for c in replay) >= 1 and not any(c[0] == "toc3d_plan_run" for c in first)
        lanes = {c[-1] for c in record if isinstance(c[-1], int) and c[-1] >= LANE0}
        assert lanes and max(lanes) < LANE0 + 64, f"{name}: the recording names its lanes"


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name):
    got, want = trace(CASES[name]), GOLDEN[name]
    assert len(got) == len(want) == FORWARDS
    for which, g, w in zip(("first", "second", "third"), got, want):
        assert [c[0] for c in g] == [c[0] for c in w], f"{name}, {which} forward: other entry points, or another order"
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"{name}, {which} forward, call {i} ({b[0]}): {a} != {b}"
