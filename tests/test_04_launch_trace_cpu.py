"""The launch sequence of every engine mode, pinned without a GPU: the C-ABI calls of one forward (+ backward) of each case of
tests/launch_trace.py -- entry points in order, every scalar, every tensor argument as (buffer, byte offset, dtype), every field of the
epilogue structs -- equal tests/golden/launch_trace.json (tools/gen_launch_trace_golden.py).  A host-side refactor of hip/engine.py
leaves every trace as it is; a change that moves a launch shows in the golden file's diff, one call per line."""
import pytest

from helpers import load_golden
from launch_trace import CASES, trace_case


@pytest.fixture(scope="module")
def golden():
    return load_golden("launch_trace")


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_trace(case, golden, monkeypatch):
    got, want = trace_case(case, monkeypatch.setattr), golden[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: call {i} differs"
    assert len(got) == len(want), f"{case}: {len(got)} calls, golden has {len(want)}"
