"""``FusedAdamW``'s eager step paths, pinned without a GPU: per scenario of tests/optim_trace.py -- the three modes, a sharded rank,
an engine rebuild, a checkpoint, a tensor in no flat buffer -- the C-ABI calls in order with every argument, and after every step the
state the host can see, equal tests/golden/optim_trace.json (tools/gen_optim_trace_golden.py).  A refactor of hip/optim.py leaves the
file as it is; a change that moves a launch shows in its diff, one call per line."""
import json

import pytest

from helpers import load_golden
from optim_trace import SCENARIOS, trace


@pytest.fixture(scope="module")
def golden():
    return load_golden("optim_trace")


def test_golden_holds_exactly_the_scenarios(golden):
    assert sorted(golden) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_optim_trace(name, golden, monkeypatch):
    from bioscanclip.hip.optim import FusedAdamW
    got, want = json.loads(json.dumps(trace(name, FusedAdamW, monkeypatch.setattr))), golden[name]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}: call {i} differs"
    assert len(got["calls"]) == len(want["calls"]), f"{name}: {len(got['calls'])} calls, golden has {len(want['calls'])}"
    assert got["raises"] == want["raises"]
    for k, (g, w) in enumerate(zip(got["steps"], want["steps"])):
        assert g == w, f"{name}: state after step {k + 1} differs"
    assert len(got["steps"]) == len(want["steps"])
