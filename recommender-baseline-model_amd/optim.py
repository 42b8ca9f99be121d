"""The fused, device-side optimizers over a FlatParams buffer, their scheduler and their checkpoint formats (torch's
state_dict layouts).  Which flat ranges a step launches over, and which keep their gradient, is decided in ONE place,
``plan``; ``FusedOptimizer.step`` issues that plan, an optimizer supplies the launch of one range (``_step``)."""
import math

import torch

from . import ops
from .flat import ALIGN


def complement(cuts, numel, overlap="ranges overlap"):
    """The gaps [(lo, hi)] the ranges `cuts` leave in [0, numel), ascending; ValueError(overlap) when two overlap."""
    gaps, a = [], 0
    for lo, hi in sorted(tuple(c) for c in cuts) + [(numel, numel)]:
        if lo < a:
            raise ValueError(overlap)
        if lo > a:
            gaps.append((a, lo))
        a = hi
    return gaps


def plan(numel, ranges=None, keep=None, sparse=None, weight_decay=0.0):
    """The dense launches of one step over a flat buffer of `numel` elements, in order: [(lo, hi, zero_grad)].
    ranges = [(lo, hi)]: exactly those slices, gradient cleared (a vocabulary-sharded rank skips the output rows other
    ranks own).  `keep` IS IGNORED WHEN `ranges` IS GIVEN: the data-parallel step passes both and its ranges win (the
    kept slice's gradient is cleared like every other).  keep = (lo, hi) alone: the whole buffer, that slice in a
    launch of its own that leaves its gradient in place.  Neither: one launch over everything.  sparse = [(lo, rows,
    d, ..)], with neither of them and weight_decay == 0: the complement of those tables; a table runs to the end of its
    alignment padding (FlatParams.ALIGN: zero in every buffer under either rule), so dense ranges start 16-B aligned."""
    if sparse:
        if ranges is not None or keep is not None:
            raise ValueError("sparse tables go with neither ranges nor keep")
        if weight_decay != 0.0:
            raise ValueError("sparse tables need weight_decay == 0: the decay has no meaning for a skipped row")
        cuts = []
        for lo, rows, d, *_ in sparse:
            lo, n = int(lo), int(rows) * int(d)
            if lo % ALIGN or lo < 0 or n <= 0 or lo + n > numel:
                raise ValueError(f"sparse table (lo={lo}, rows={rows}, d={d}) is not a parameter of the flat buffer")
            cuts.append((lo, min(lo + -(-n // ALIGN) * ALIGN, numel)))
        return [(lo, hi, True) for lo, hi in complement(cuts, numel, "sparse tables overlap")]
    if ranges is not None or keep is None:
        return [(lo, hi, True) for lo, hi in (ranges or [(0, numel)])]
    assert 0 < keep[0] < keep[1] <= numel and keep[0] % 4 == 0 and keep[1] % 4 == 0, keep
    return sorted([(lo, hi, True) for lo, hi in complement([keep], numel)] + [(*keep, False)])


class FusedOptimizer:
    """What FusedAdam and FusedSGD share: the learning-rate hook and the skeleton of a step."""

    # (table lo, rows, log2 d, row marks, epoch): a table whose gradient rows only the marked item gradient writes --
    # FusedAdam's sweep skips the gradient loads of the rows it did not stamp (rs_adam_*_marked)
    marks = None
    momentum = 0.0
    NO_SPARSE = None    # why step(sparse=...) is refused, for an optimizer without the lazy rule

    def set_lr(self, lr):
        """StepLR hook (BS/trainers/base.py:40,87): lives on the device, so graph replays see it."""
        self.hyper[0] = lr

    def _views(self, lo, hi, *bufs):
        """[lo, hi) of the parameters, the gradient, `bufs` and the bf16 copy (None where a buffer is)."""
        f = self.flat
        return [None if b is None else b[lo:hi] for b in (f.data, f.grad) + bufs + (f.bf16,)]

    def _moments_out(self, slices):
        """{i: {key: parameter i's part of that moment buffer, on the host}} over slices = [(parameter, offset)]."""
        return {i: {k: b[off:off + p.numel()].view(p.shape).detach().cpu().clone()
                    for k, b in zip(self.STATE_KEYS, self.moment_buffers())} for i, (p, off) in enumerate(slices)}

    def _moments_in(self, sd, slices):
        """Fill the moment buffers from sd's per-parameter states (zero where torch holds none yet); -> those used."""
        held = []
        for b in self.moment_buffers():
            b.zero_()
        for i, (p, off) in enumerate(slices):
            st = sd["state"].get(i)
            if st and st.get(self.STATE_KEYS[0]) is not None:
                for k, b in zip(self.STATE_KEYS, self.moment_buffers()):
                    b[off:off + p.numel()].copy_(st[k].reshape(-1))
                held.append(st)
        return held

    def step(self, grad_divisor=None, seed_base=None, ranges=None, transposed=None, loss=None, keep=None,
             sparse=None):
        """One update; also clears the gradient buffer (the next step accumulates from zero) and advances the dropout
        step seed when given.  ranges / keep / sparse: plan().  The first range's launch also prepares the step's
        scalars and forms loss = (sum, out): out = sum / grad_divisor; transposed (the SAS block weights' transposed
        bf16 copies) rides in it, and it must cover those matrices.  keep: a slice the backward OVERWRITES every step
        (BERT's out.weight / out.bias with a large vocabulary): no zero written by this sweep, none read back by the
        next step's dE GEMM (2 GB per step at 1M items).  sparse: FusedAdam's lazy rule (_step_rows)."""
        if sparse and self.NO_SPARSE:
            raise ValueError(self.NO_SPARSE)
        segs = plan(self.flat.numel, ranges, keep, sparse, self.weight_decay)
        prepare = dict(seed_base=seed_base, transposed=transposed, loss_sum=loss[0] if loss else None,
                       loss_out=loss[1] if loss else None)
        if not segs:     # nothing dense (sparse tables cover the buffer): the step's scalars by their own launch
            self._prepare(grad_divisor, seed_base)
        for k, (lo, hi, zg) in enumerate(segs):
            self._step(lo, hi, zg, grad_divisor, prepare if k == 0 else None)
        for table in sparse or ():
            self._step_rows(*table)


class FusedAdam(FusedOptimizer):
    """Device-side torch.optim.Adam over a FlatParams buffer (rs_adam_prepare_step / rs_adam_step)."""
    STATE_KEYS = ("exp_avg", "exp_avg_sq")      # torch.optim.Adam's names of moment_buffers()

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        dev = flat.device
        self.flat = flat
        self.m = torch.zeros(flat.numel, dtype=torch.float32, device=dev)
        self.v = torch.zeros(flat.numel, dtype=torch.float32, device=dev)
        # [t, lr/bc1, sqrt(bc2), grad scale, -, -, -, arrival counters of rs_adam_prepare_step (state[7],
        # state[16 + 16 k], k < 8)]
        self.state = torch.zeros(144, dtype=torch.float64, device=dev)
        self.hyper = torch.tensor([lr, betas[0], betas[1], eps, weight_decay], dtype=torch.float64, device=dev)
        self.weight_decay = float(weight_decay)     # host copy: step(sparse=...) refuses a non-zero decay

    def moment_buffers(self):
        return [self.m, self.v]

    def _marks(self, lo, hi):
        if self.marks is None:
            return None
        tlo, rows, dshift, rm, ep = self.marks
        if hi <= tlo or lo >= tlo + (rows << dshift):
            return None
        return rm, ep, tlo - lo, rows, dshift

    def _sparse_segments(self, sparse):
        """The dense launches' ranges beside the sparse tables: plan()'s complement of the tables."""
        return plan(self.flat.numel, sparse=sparse, weight_decay=self.weight_decay)

    def _prepare(self, grad_divisor, seed_base):
        ops.adam_prepare(self.state, self.hyper, grad_divisor, seed_base)

    def _step(self, lo, hi, zero_grad, grad_divisor, prepare=None):
        """One range of step(); prepare: the first range's extra arguments (rs_adam_prepare_step), else rs_adam_step."""
        if prepare is None:
            return self.step_range(lo, hi, zero_grad)
        p, g, m, v, bf = self._views(lo, hi, self.m, self.v)
        ops.adam_prepare_step(p, g, m, v, bf, self.state, self.hyper, zero_grad=zero_grad, grad_divisor=grad_divisor,
                              tbase=lo, marks=self._marks(lo, hi), **prepare)

    def _step_rows(self, lo, rows, d, lst, cnt):
        """One table of step(sparse=[(lo, rows, d, rows_list, count)]): [rows][d] at flat offset lo, under the LAZY
        rule: only the rows rows_list[:count] (ops.unique_rows: int32 device list and count, distinct ids) are
        updated, by rs_adam_rows after the preparing launch, with the dense sweep's arithmetic and this step's scalars;
        every other row of p / m / v / the bf16 copy stays bit for bit, its gradient (zero by contract) neither read
        nor written.  With every row listed every step this is the dense step bit for bit.  Against torch's SparseAdam
        only the place of eps differs: denom = sqrt(v) / sqrt(bc2) + eps and step size lr / bc1, as the dense kernel."""
        shp = (rows, d) if d > 1 else (rows,)
        p, g, m, v, bf = (None if t is None else t.view(shp) for t in self._views(lo, lo + rows * d, self.m, self.v))
        ops.adam_rows(lst, cnt, p, g, m, v, bf, self.state, self.hyper, zero_grad=True)

    def step_keep_early(self, keep, max_wg=None, zero_grad=False):
        """The first part of a step whose `keep` range is final before the rest of the backward (BERT's out.weight /
        out.bias, after the head's dE / dh): rs_adam_prepare (t += 1 and the step's scalars; no seed advance -- the
        backward still draws this step's dropout masks) and that range's update, gradient left in place.  step_rest()
        finishes the step: the same per-element math as step(keep=...), bit for bit."""
        ops.adam_prepare(self.state, self.hyper)
        self.step_range(*keep, zero_grad=zero_grad, max_wg=max_wg)

    def step_range(self, lo, hi, zero_grad=True, max_wg=None):
        """rs_adam_step over [lo, hi) with the step's scalars already prepared (a step_keep_early step)."""
        p, g, m, v, bf = self._views(lo, hi, self.m, self.v)
        ops.adam_step(p, g, m, v, bf, self.state, self.hyper, zero_grad=zero_grad, max_wg=max_wg,
                      marks=self._marks(lo, hi))

    def step_rest(self, keep, seed_base=None, done=()):
        """The rest of a step_keep_early step: every range outside `keep` and the ranges in `done` (already updated
        by step_range) with the gradient cleared, then the seed."""
        for lo, hi in complement([keep, *done], self.flat.numel):
            self.step_range(lo, hi)
        if seed_base is not None:
            ops.seed_advance(seed_base)

    def state_dict(self, model_params, slices):
        """torch.optim.Adam's state_dict() layout (param_groups from a real Adam over the same parameters;
        per-parameter 'step', 'exp_avg', 'exp_avg_sq').  slices: (parameter, flat offset) in model_params' order."""
        hy = self.hyper.cpu().tolist()
        sd = torch.optim.Adam(model_params, lr=hy[0], betas=(hy[1], hy[2]), eps=hy[3], weight_decay=hy[4]).state_dict()
        step = float(self.state[0].item())
        if step > 0:
            sd["state"] = {i: {"step": torch.tensor(step), **st} for i, st in self._moments_out(slices).items()}
        return sd

    def load_state_dict(self, sd, slices, captured=False):
        g = sd["param_groups"][0]
        if "betas" not in g:
            raise ValueError("optimizer='adam' cannot load this optimizer state: its param_groups have no 'betas' (a "
                             "torch.optim.SGD checkpoint loads into a step built with optimizer='sgd')")
        self.weight_decay = float(g["weight_decay"])
        self.hyper.copy_(torch.tensor([g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]],
                                      dtype=torch.float64))
        steps = {float(st["step"]) for st in self._moments_in(sd, slices)}
        if len(steps) > 1:
            raise ValueError("per-parameter Adam step counts differ; the fused optimizer keeps one")
        self.state.zero_()
        self.state[0] = steps.pop() if steps else 0.0


class FusedSGD(FusedOptimizer):
    """Device-side torch.optim.SGD(params, lr, momentum=, weight_decay=) over a FlatParams buffer (rs_sgd_step): the
    reference's other optimizer (BS/trainers/base.py:229-233; dampening 0, nesterov False).  hyper[0] is the rate, so
    FusedStepLR drives it through set_lr as it drives FusedAdam; state[0] is the device step count.  No row marks."""

    MAX_WG = 8192      # rs_adam_step's grid bound
    NO_SPARSE = "FusedSGD has no sparse (touched-rows-only) rule: the lazy rule is Adam's"
    # torch.optim.SGD's state_dict carries no step count: the device count (kernel stamps, resumed runs) travels in
    # this extra param_groups key, which torch.optim.SGD.load_state_dict keeps and never reads
    SGD_STEP_KEY = "fused_step"
    STATE_KEYS = ("momentum_buffer",)

    def __init__(self, flat, lr, momentum=0.0, weight_decay=0.0):
        dev = flat.device
        self.flat = flat
        self.momentum = float(momentum)
        self.weight_decay = float(weight_decay)
        # the momentum buffer, zero-initialised: torch's first-step rule (buf = grad.clone()) falls out of the update
        self.buf = torch.zeros(flat.numel, dtype=torch.float32, device=dev) if self.momentum != 0 else None
        self.state = torch.zeros(8, dtype=torch.float64, device=dev)
        self.hyper = torch.tensor([lr, self.momentum, self.weight_decay], dtype=torch.float64, device=dev)

    def moment_buffers(self):
        return [self.buf] if self.buf is not None else []

    def _step(self, lo, hi, zero_grad, grad_divisor, prepare=None):
        p, g, buf, bf = self._views(lo, hi, self.buf)
        ops.sgd_step(p, g, buf, bf, self.state, self.hyper, zero_grad=zero_grad, prepare=prepare is not None,
                     grad_divisor=grad_divisor, tbase=lo, max_wg=self.MAX_WG, **(prepare or {}))

    def state_dict(self, model_params, slices):
        """torch.optim.SGD's state_dict() layout: param_groups from a real SGD over the same parameters plus
        SGD_STEP_KEY; state[i] = {'momentum_buffer'} once a step has run with a non-zero momentum, else empty."""
        lr, mom, wd = self.hyper.cpu().tolist()
        sd = torch.optim.SGD(model_params, lr=lr, momentum=mom, weight_decay=wd).state_dict()
        step = float(self.state[0].item())
        sd["param_groups"][0][self.SGD_STEP_KEY] = step
        if step > 0 and self.buf is not None:
            sd["state"] = self._moments_out(slices)
        return sd

    def load_state_dict(self, sd, slices, captured=False):
        g = sd["param_groups"][0]
        if "betas" in g or "momentum" not in g:
            raise ValueError("optimizer='sgd' cannot load this optimizer state: its param_groups are not "
                             "torch.optim.SGD's (an Adam checkpoint loads into a step built with optimizer='adam')")
        if g.get("dampening", 0) != 0:
            raise ValueError(f"dampening must be 0 (the loaded optimizer state has {g['dampening']}): the fused SGD "
                             "has none")
        if g.get("nesterov", False):
            raise ValueError("nesterov must be False (the loaded optimizer state has nesterov=True): the fused SGD "
                             "has none")
        mom = float(g["momentum"])
        if not math.isfinite(mom) or mom < 0:
            raise ValueError(f"momentum must be a finite number >= 0 (the loaded optimizer state has {mom})")
        if (mom != 0) != (self.buf is not None) and captured:
            # a captured graph holds the buffer's pointer and the kernel chosen for its presence: a new or a dropped
            # buffer would leave the graph on the old one
            raise ValueError(f"the loaded optimizer state has momentum={mom}, the captured step graphs were built "
                             f"with momentum={self.momentum}: load it before capture(), or build the step with "
                             "that momentum")
        if mom != 0 and self.buf is None:
            self.buf = torch.zeros(self.flat.numel, dtype=torch.float32, device=self.flat.device)
        elif mom == 0:
            self.buf = None
        self.momentum = mom
        self.weight_decay = float(g["weight_decay"])
        self.hyper.copy_(torch.tensor([g["lr"], mom, g["weight_decay"]], dtype=torch.float64))
        seen = self._moments_in(sd, slices) if self.buf is not None else []
        self.state.zero_()
        # a checkpoint torch.optim.SGD wrote has no count: 1 when it holds buffers (some step ran), else 0
        self.state[0] = float(g.get(self.SGD_STEP_KEY, 1.0 if seen else 0.0))


class FusedStepLR:
    """``torch.optim.lr_scheduler.StepLR(optimizer, step_size, gamma)`` for a FusedAdam or FusedSGD (BS/trainers/
    base.py:40, stepped once per epoch at :87): every ``step_size``-th ``step()`` multiplies the learning rate by
    ``gamma`` -- chained in Python floats exactly as torch's StepLR forms it -- and writes it into the optimizer's
    device hyperparameters, so captured step graphs replayed afterwards use it without re-capture."""

    def __init__(self, optimizer, step_size, gamma=0.1):
        self.optimizer = getattr(optimizer, "opt", optimizer)      # given a FusedTrainStep: its optimizer
        self.step_size = int(step_size)
        self.gamma = float(gamma)
        self.base_lr = float(self.optimizer.hyper[0].item())
        self.lr = self.base_lr
        self.last_epoch = 0

    def step(self):
        self.last_epoch += 1
        if self.last_epoch % self.step_size == 0:
            self.lr = self.lr * self.gamma
            self.optimizer.set_lr(self.lr)

    def get_last_lr(self):
        return [self.lr]

    def state_dict(self):
        return {"step_size": self.step_size, "gamma": self.gamma, "base_lrs": [self.base_lr],
                "last_epoch": self.last_epoch, "_last_lr": [self.lr]}
