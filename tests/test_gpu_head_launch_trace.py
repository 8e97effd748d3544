"""GPU: the head's four modules hand the library what tests/golden/head_launch_traces.json recorded -- every ``lib.call`` of the first forward (weight packing, the
learned queries' half, the frame) and of the second (the frame alone), entry by entry and argument by argument: dtype codes, epilogues, tile variants, M / N / K,
leading dimensions, eps, tensor dtypes and shapes (addresses as "ptr").  Cases, normalisation and the recorder are tools/gen_head_launch_traces.py's, which wrote
the file; a change that alters the launches on purpose regenerates it."""
import json

import pytest

from tools.gen_head_launch_traces import PATH, cases, trace

pytestmark = pytest.mark.gpu
CASES = cases()
with open(PATH) as fh:
    GOLDEN = json.load(fh)


def test_the_recorded_cases_are_the_generators():
    assert sorted(GOLDEN) == sorted(CASES)
    assert all(len(t) == 2 and t[0] and t[1] and len(t[0]) > len(t[1]) for t in GOLDEN.values()), "two lists per case, the first with the pack launches on top"


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name):
    got, want = trace(CASES[name]), GOLDEN[name]
    for which, g, w in zip(("first", "second"), got, want):
        assert [c[0] for c in g] == [c[0] for c in w], f"{name}, {which} forward: other entry points, or another order"
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"{name}, {which} forward, call {i} ({b[0]}): {a} != {b}"
