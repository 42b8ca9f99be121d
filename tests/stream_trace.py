"""Recorder of a training step's stream choreography, and the cases tests/test_step_streams_gpu.py pins.

While installed, the recorder notes every kernel entry issued through ``rbm_amd.ops.call`` with the stream it went to,
and every ``torch.cuda.Event.record`` / ``torch.cuda.Stream.wait_event`` / ``torch.cuda.Stream.wait_stream``:

    ("launch", entry name, stream label)
    ("record", event number, stream label)
    ("wait_event", waiting stream label, event number)
    ("wait_stream", waiting stream label, waited stream label)

Streams are labelled s0, s1, ... and events numbered 0, 1, ... in order of first appearance within one trace; a
stream's identity is its handle, an event's the object.  ``wait_stream`` is one entry (torch forms it from an event of
its own, which is not listed).  Only torch's own primitives and ``ops.call`` are patched, so the recorder runs on any
revision of the package; tests/golden/step_traces.json holds the traces of the revision before the side-branch helper
(the optimizer variants in CASES: of the revision before the optimizers moved into rbm_amd.optim; the row-head cases at
the end of CASES: of the revision before the row-head protocol, rbm_amd.models.sas_model.heads).
"""
import argparse

import numpy as np
import torch


class Recorder:
    def __init__(self, monkeypatch):
        from rbm_amd import ops
        self.trace, self._streams, self._events, self._depth = [], {}, {}, 0
        call, record = ops.call, torch.cuda.Event.record
        wait_event, wait_stream = torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

        def traced_call(name, *a):
            self._add("launch", name, self._stream(torch.cuda.current_stream()))
            return call(name, *a)

        def traced_record(ev, stream=None):
            st = stream if stream is not None else torch.cuda.current_stream()
            self._add("record", self._event(ev), self._stream(st))
            return record(ev, stream)

        def traced_wait_event(st, ev):
            self._add("wait_event", self._stream(st), self._event(ev))
            return wait_event(st, ev)

        def traced_wait_stream(st, other):
            self._add("wait_stream", self._stream(st), self._stream(other))
            self._depth += 1
            try:
                return wait_stream(st, other)
            finally:
                self._depth -= 1
        monkeypatch.setattr(ops, "call", traced_call)
        monkeypatch.setattr(torch.cuda.Event, "record", traced_record)
        monkeypatch.setattr(torch.cuda.Stream, "wait_event", traced_wait_event)
        monkeypatch.setattr(torch.cuda.Stream, "wait_stream", traced_wait_stream)

    def _add(self, *entry):
        if not self._depth:
            self.trace.append(list(entry))

    def _stream(self, st):
        return self._streams.setdefault(st.cuda_stream, f"s{len(self._streams)}")

    def _event(self, ev):
        if self._depth:
            return None
        # the event is held for the length of the trace: a freed one's id could come back as another event's
        return self._events.setdefault(id(ev), (len(self._events), ev))[0]

    def take(self):
        """The trace so far; the next one starts with fresh labels."""
        out, self.trace = self.trace, []
        self._streams, self._events = {}, {}
        return out


def streams(trace):
    """The stream labels of a trace."""
    out = set()
    for e in trace:
        out.update(x for x in e[1:] if isinstance(x, str) and x[0] == "s" and x[1:].isdigit())
    return out


# ------------------------------------------------------------------ the cases
def _sas(d, dtype, loss, turnaround="1", K=0, N=0, ce_rows=None, logq=False, **step_kw):
    def make(monkeypatch):
        import rbm_amd.data as synth
        from rbm_amd.models import model_factory
        from rbm_amd.train_step import FusedTrainStep
        monkeypatch.setenv("RS_SAS_TURNAROUND_FUSE", turnaround)
        if ce_rows is not None:
            monkeypatch.setenv("RS_SAS_CE_ROWS", ce_rows)
        V, T, B = 200, 16, 4
        torch.manual_seed(0)
        a = argparse.Namespace(model_code="sas", num_items=V, max_len=T, device="cuda", sas_hidden_units=d,
                               sas_num_blocks=2, sas_heads=1, sas_dropout=0.2, l2_emb=0.0, rs_dtype=dtype,
                               sas_loss=loss, sas_shared_negs=K, sas_negs=N)
        kw = dict(step_kw)
        if logq:        # a normalised proposal over the V + 1 rows (entry 0 is never read)
            kw["logq"] = torch.log_softmax(torch.arange(V + 1, dtype=torch.float32), 0).cuda()
        tr = FusedTrainStep(model_factory(a), lr=1e-3, **kw)
        rng = np.random.default_rng(7)
        batches = []
        for _ in range(2):
            seq, pos, neg = (torch.from_numpy(x).cuda() for x in synth.sas_batch(rng, B, T, V))
            if loss == "sampled_ce":
                neg = torch.from_numpy(rng.integers(1, V + 1, K)).cuda()
            if loss == "gbce":
                neg = torch.from_numpy(rng.integers(1, V + 1, (B, T, N))).cuda()
            batches.append((seq, pos, neg))
        return tr, batches
    return make


def _bert(V, T, d, L, h, B, loss=None, K=0, **step_kw):
    def make(monkeypatch):
        import rbm_amd.data as synth
        from rbm_amd.models import model_factory
        from rbm_amd.train_step import FusedTrainStep
        torch.manual_seed(0)
        a = argparse.Namespace(model_code="bert", num_items=V, max_len=T, device="cuda", bert_hidden_units=d,
                               bert_num_blocks=L, bert_num_heads=h, bert_dropout=0.1, bert_hidden_dropout=0.1,
                               bert_mask_prob=0.2, model_init_seed=0, rs_dtype="bf16")
        m = model_factory(a)
        m.train()
        tr = FusedTrainStep(m, lr=1e-3, loss=loss, **step_kw)
        rng = np.random.default_rng(7)
        batches = []
        for _ in range(2):
            b = tuple(torch.from_numpy(x).cuda() for x in synth.bert_batch(rng, B, T, V, mask_prob=0.3))
            if loss == "sampled_ce":
                b += (torch.from_numpy(rng.integers(1, V + 1, K)).cuda(),)
            batches.append(b)
        return tr, batches
    return make


# the smallest catalogue whose head gradient the step overwrites whole (BERTEngine.overwritten_grads: V1 d >= 2^24)
BIG_V = (1 << 24) // 64 - 1

CASES = {
    "sas_bce": _sas(64, "bf16", "bce"),
    "sas_bce_no_turnaround": _sas(64, "bf16", "bce", turnaround="0"),
    "sas_ce": _sas(64, "bf16", "ce"),
    "sas_sampled_ce": _sas(64, "bf16", "sampled_ce", K=16),
    "sas_fp32_bce": _sas(50, "fp32", "bce"),
    "bert_ce": _bert(300, 24, 64, 1, 2, 8),
    "bert_sampled_ce": _bert(300, 24, 64, 1, 2, 8, loss="sampled_ce", K=50),
    "bert_big_vocab": _bert(BIG_V, 8, 64, 1, 2, 2),
    # the optimizer variants (recorded at the revision before the optimizers moved into rbm_amd.optim)
    "sas_bce_sgd_momentum": _sas(64, "bf16", "bce", optimizer="sgd", momentum=0.9),
    "sas_bce_sparse_tables": _sas(64, "bf16", "bce", table_optim="sparse"),
    "sas_bce_clip": _sas(64, "bf16", "bce", max_grad_norm=1.0),
    "bert_sampled_ce_sparse_clip": _bert(300, 24, 64, 1, 2, 8, loss="sampled_ce", K=50, table_optim="sparse",
                                         max_grad_norm=1.0),
    # the row heads' other forms (recorded at the revision before the row-head protocol, models/sas_model/heads.py)
    "sas_gbce": _sas(64, "bf16", "gbce", N=3),
    "sas_gbce_sparse_tables": _sas(64, "bf16", "gbce", N=3, table_optim="sparse"),
    "sas_sampled_ce_logq": _sas(64, "bf16", "sampled_ce", K=16, logq=True),
    "sas_ce_composed_rows": _sas(64, "bf16", "ce", ce_rows="0"),
    "sas_fp32_ce": _sas(50, "fp32", "ce"),
    "sas_fp32_sampled_ce": _sas(64, "fp32", "sampled_ce", K=16),
    "sas_fp32_gbce": _sas(50, "fp32", "gbce", N=2),
}


def run_case(name, monkeypatch):
    """(trainer, [trace of the first step, trace of the second]): two consecutive eager steps of the case."""
    tr, batches = CASES[name](monkeypatch)
    torch.cuda.synchronize()
    rec = Recorder(monkeypatch)
    traces = []
    for b in batches:
        tr.step(*b)
        traces.append(rec.take())
    torch.cuda.synchronize()
    return tr, traces
