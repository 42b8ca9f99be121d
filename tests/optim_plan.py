"""Recorder of the fused optimizers' launch plans, and the cases tests/test_optim_plan.py pins.

While installed, the recorder replaces the optimizer entries of ``rbm_amd.ops`` (adam_prepare, adam_prepare_step,
adam_step, adam_rows, sgd_step, seed_advance), so FusedAdam / FusedSGD driven over a CPU stand-in of the flat buffer
reach no kernel, and notes for every call: the entry, the [lo, hi) of ``p`` inside the flat buffer (from its storage
offset and length; the gradient, moment and bf16 slices must name the same range), zero_grad / prepare / tbase /
max_wg, which of the optional pointers were passed, the integers of ``marks`` and the row shape of adam_rows.

The classes are imported from ``rbm_amd.train_step``, so the file runs on any revision of the package;
tests/golden/optim_plans.json holds the plans of the revision before the optimizers moved into rbm_amd.optim:

    python tests/optim_plan.py > tests/golden/optim_plans.json
"""
import contextlib
import json
import os
import sys
from types import SimpleNamespace

import torch

NUMEL = 4096
OPTIONAL = ("grad_divisor", "seed_base", "transposed", "loss_sum", "loss_out")


def _span(t):
    return [t.storage_offset(), t.storage_offset() + t.numel()]


class Recorder:
    def __init__(self):
        self.plan = []

    def _sweep(self, entry, p, others, kw):
        rec = {"entry": entry, "range": _span(p), "bf16": others[-1] is not None}
        for t in others:
            assert t is None or _span(t) == rec["range"], (entry, rec["range"], _span(t))
        for k in ("zero_grad", "prepare", "tbase", "max_wg"):
            if k in kw:
                rec[k] = kw[k] if kw[k] is None else int(kw[k])
        rec["passed"] = [k for k in OPTIONAL if kw.get(k) is not None]
        if "marks" in kw:
            rec["marks"] = None if kw["marks"] is None else [int(x) for x in kw["marks"][2:]]
        self.plan.append(rec)
        return rec

    def adam_prepare(self, state, hyper, grad_divisor=None, seed_base=None):
        passed = [k for k, x in (("grad_divisor", grad_divisor), ("seed_base", seed_base)) if x is not None]
        self.plan.append({"entry": "adam_prepare", "passed": passed})

    def adam_prepare_step(self, p, g, m, v, p_bf16, state, hyper, zero_grad=False, grad_divisor=None, seed_base=None,
                          transposed=None, loss_sum=None, loss_out=None, tbase=0, marks=None):
        self._sweep("adam_prepare_step", p, (g, m, v, p_bf16),
                    dict(zero_grad=zero_grad, grad_divisor=grad_divisor, seed_base=seed_base, transposed=transposed,
                         loss_sum=loss_sum, loss_out=loss_out, tbase=tbase, marks=marks))

    def adam_step(self, p, g, m, v, p_bf16, state, hyper, zero_grad=False, max_wg=None, marks=None):
        self._sweep("adam_step", p, (g, m, v, p_bf16), dict(zero_grad=zero_grad, max_wg=max_wg, marks=marks))

    def adam_rows(self, rows, count, p, g, m, v, p_bf16, state, hyper, zero_grad=False, max_wg=None):
        rec = self._sweep("adam_rows", p, (g, m, v, p_bf16), dict(zero_grad=zero_grad, max_wg=max_wg))
        for t in (g, m, v, p_bf16):
            assert t is None or t.shape == p.shape
        rec["shape"] = list(p.shape)
        rec["list"] = [rows.numel(), count.numel()]

    def sgd_step(self, p, g, buf, p_bf16, state, hyper, zero_grad=False, prepare=False, grad_divisor=None,
                 seed_base=None, transposed=None, tbase=0, loss_sum=None, loss_out=None, max_wg=8192):
        rec = self._sweep("sgd_step", p, (g, buf, p_bf16),
                          dict(zero_grad=zero_grad, prepare=prepare, grad_divisor=grad_divisor, seed_base=seed_base,
                               transposed=transposed, tbase=tbase, loss_sum=loss_sum, loss_out=loss_out,
                               max_wg=max_wg))
        rec["buf"] = buf is not None

    def seed_advance(self, seed_base):
        self.plan.append({"entry": "seed_advance"})


@contextlib.contextmanager
def recording():
    """Install a Recorder over rbm_amd.ops' optimizer entries for the length of the block."""
    from rbm_amd import ops
    rec = Recorder()
    names = ("adam_prepare", "adam_prepare_step", "adam_step", "adam_rows", "sgd_step", "seed_advance")
    saved = {n: getattr(ops, n) for n in names}
    for n in names:
        setattr(ops, n, getattr(rec, n))
    try:
        yield rec
    finally:
        for n, fn in saved.items():
            setattr(ops, n, fn)


def flat(numel=NUMEL, bf16=True):
    """The CPU stand-in of a FlatParams buffer: what the optimizers read of it."""
    return SimpleNamespace(numel=numel, device=torch.device("cpu"), data=torch.zeros(numel), grad=torch.zeros(numel),
                           bf16=torch.zeros(numel, dtype=torch.bfloat16) if bf16 else None)


# ------------------------------------------------------------------ the cases
def _scalars():
    z = torch.zeros(1)
    return SimpleNamespace(div=z.clone(), seed=torch.zeros(1, dtype=torch.int64), lsum=z.clone(), lout=z.clone(),
                           lst=torch.zeros(8, dtype=torch.int32), cnt=torch.zeros(1, dtype=torch.int32),
                           rm=torch.zeros(64, dtype=torch.uint8), ep=torch.zeros(1, dtype=torch.uint8),
                           # a transposed spec as the engine hands it on: (device descriptors, host copy, destination);
                           # the recorded entries never look inside
                           tr=(torch.zeros(1, 6, dtype=torch.int64), [], torch.zeros(16, dtype=torch.bfloat16)))


def _adam(**kw):
    from rbm_amd.train_step import FusedAdam
    return FusedAdam(flat(**kw))


def _sgd(momentum):
    from rbm_amd.train_step import FusedSGD
    return FusedSGD(flat(), lr=0.1, momentum=momentum)


def _early(s):
    opt = _adam()
    keep = (1024, 2048)
    opt.step_keep_early(keep, max_wg=256)
    opt.step_range(64, 128, max_wg=256)
    opt.step_rest(keep, s.seed, done=[(64, 128)])


def _marked(s, **kw):
    opt = _adam()
    opt.marks = (512, 16, 5, s.rm, s.ep)
    opt.step(seed_base=s.seed, **kw)


RANGES = [(0, 512), (1024, NUMEL)]

CASES = {
    "adam_default": lambda s: _adam().step(seed_base=s.seed),
    "adam_keep": lambda s: _adam().step(seed_base=s.seed, keep=(1024, 2048)),
    "adam_keep_to_end": lambda s: _adam().step(seed_base=s.seed, keep=(1024, NUMEL)),
    "adam_ranges_divisor_loss": lambda s: _adam().step(grad_divisor=s.div, seed_base=s.seed, ranges=RANGES,
                                                       loss=(s.lsum, s.lout)),
    "adam_ranges_with_keep": lambda s: _adam().step(grad_divisor=s.div, seed_base=s.seed, ranges=RANGES,
                                                    keep=(1024, 2048)),
    "adam_sparse": lambda s: _adam().step(seed_base=s.seed, sparse=[(64, 10, 5, s.lst, s.cnt),
                                                                    (1024, 3, 1, s.lst, s.cnt)]),
    "adam_sparse_whole_buffer": lambda s: _adam().step(grad_divisor=s.div, seed_base=s.seed,
                                                       sparse=[(0, NUMEL, 1, s.lst, s.cnt)]),
    "adam_early_head": _early,
    "adam_marks_keep": lambda s: _marked(s, keep=(1024, 2048)),
    "adam_marks_ranges_inside_table": lambda s: _marked(s, ranges=[(0, 256), (768, 2048), (2048, NUMEL)]),
    "adam_transposed_bf16": lambda s: _adam().step(seed_base=s.seed, transposed=s.tr),
    "adam_no_bf16": lambda s: _adam(bf16=False).step(seed_base=s.seed, keep=(1024, 2048)),
}
for _name, _mom in (("sgd", 0.0), ("sgd_momentum", 0.9)):
    CASES.update({
        f"{_name}_default": lambda s, m=_mom: _sgd(m).step(seed_base=s.seed),
        f"{_name}_keep": lambda s, m=_mom: _sgd(m).step(seed_base=s.seed, keep=(1024, 2048)),
        f"{_name}_ranges_loss": lambda s, m=_mom: _sgd(m).step(grad_divisor=s.div, seed_base=s.seed, ranges=RANGES,
                                                               loss=(s.lsum, s.lout)),
        f"{_name}_transposed": lambda s, m=_mom: _sgd(m).step(seed_base=s.seed, transposed=s.tr),
    })


def run_case(name):
    """The recorded plan of one case: the list of its launches in issue order."""
    with recording() as rec:
        CASES[name](_scalars())
    return rec.plan


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    json.dump({name: run_case(name) for name in CASES}, sys.stdout, indent=1)
    sys.stdout.write("\n")
