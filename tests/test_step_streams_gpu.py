"""The stream choreography of a training step (engine_util.SideBranch: which entry goes to which stream, where the
branches fork and join), pinned as a trace: two consecutive eager steps of each case of tests/stream_trace.py -- the
first takes the `_wT is None` / `_side_refreshed` path, the second the optimizer-written transposes -- must issue
exactly the launches, event records and waits stored in tests/golden/step_traces.json, which the revision before the
helper produced (the later cases: the revisions named in stream_trace's docstring).  And engine_util.new_stream:
distinct streams at every offset of torch's round-robin pool."""
import json
import os

import pytest
import torch

import stream_trace
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _golden():
    with open(os.path.join(GOLDEN, "step_traces.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", list(stream_trace.CASES))
def test_step_trace_equals_the_stored_one(name, monkeypatch):
    tr, traces = stream_trace.run_case(name, monkeypatch)
    want = _golden()[name]
    assert len(traces) == len(want) == 2
    for k, (got, exp) in enumerate(zip(traces, want)):
        for i, (g, e) in enumerate(zip(got, exp)):
            assert g == e, f"step {k}, entry {i}: {g} != {e}"
        assert len(got) == len(exp), f"step {k}: {len(got)} entries, stored {len(exp)}"
    if name in ("sas_fp32_bce", "sas_fp32_ce", "sas_fp32_gbce", "sas_fp32_sampled_ce"):
        # the unfused path: one stream (sas_fp32_sampled_ce too -- the revision before the row-head protocol recorded
        # its head table gradient on the main stream, after the LayerNorm backward)
        assert all(stream_trace.streams(t) == {"s0"} for t in traces)
    if name == "bert_big_vocab":
        # the early head and token-table Adam updates run on the optimizer's branch: a third stream
        assert tr._early_ok and tr.engine.overwritten_grads() is not None
        assert all(len(stream_trace.streams(t)) == 3 for t in traces)


def test_new_stream_is_distinct_at_every_pool_offset():
    """torch hands out its 32 pool streams per priority round-robin: at each of 33 consecutive offsets, three draws
    are distinct from one another and from the current stream."""
    from rbm_amd.engine_util import new_stream
    dev = torch.device("cuda", torch.cuda.current_device())
    for _ in range(33):
        torch.cuda.Stream()
        a = new_stream(dev)
        b = new_stream(dev, [a])
        c = new_stream(dev, [a, b])
        handles = [s.cuda_stream for s in (a, b, c, torch.cuda.current_stream())]
        assert len(set(handles)) == 4, handles
