"""Helpers shared by the SAS and BERT engines."""
import contextlib

import numpy as np
import torch


def compute_dtype(args):
    """``args.rs_dtype``: 'fp32' (default: the reference's precision, parity mode) or 'bf16'."""
    name = str(getattr(args, "rs_dtype", "fp32") or "fp32").lower()
    if name in ("fp32", "float32", "f32"):
        return torch.float32
    if name in ("bf16", "bfloat16"):
        return torch.bfloat16
    raise ValueError(f"rs_dtype must be fp32 or bf16, got {name!r}")


def as_ids(x, device):
    """numpy / list / tensor -> contiguous int64 device tensor (the reference's
    ``torch.LongTensor(x).to(device)``, BS/models/sas_model/sas.py:60,93-94)."""
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=torch.int64, non_blocking=True)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to(device, non_blocking=True)
    return t.contiguous()


def require_cuda(device):
    if torch.device(device).type != "cuda":
        raise RuntimeError(
            "rbm_amd runs the training hot path only through its HIP kernels (librecsys_hip.so); "
            "set args.device='cuda' (there is no CPU fallback)")


NEG_DISTS = ("uniform", "popular")
SCE_INDEX_ROWS = 32769      # one past the largest table the item index counting-sorts (itemgrad.hip)


def neg_dist_args(args, prefix, loss):
    """(dist, alpha) from ``args.<prefix>_neg_dist`` ('uniform', the default, or 'popular') and
    ``args.<prefix>_neg_alpha`` (default 1.0): the proposal the sampled softmax's shared candidates come from.
    'popular' describes those candidates alone, so it needs ``<prefix>_loss = 'sampled_ce'``."""
    dist = str(getattr(args, prefix + "_neg_dist", None) or "uniform")
    if dist not in NEG_DISTS:
        raise ValueError(f"{prefix}_neg_dist must be one of {NEG_DISTS}, got {dist!r}")
    if dist == "popular" and loss != "sampled_ce":
        raise ValueError(f"{prefix}_neg_dist='popular' needs {prefix}_loss='sampled_ce' (it draws the shared candidates)")
    alpha = getattr(args, prefix + "_neg_alpha", None)
    alpha = 1.0 if alpha is None else float(alpha)
    if not np.isfinite(alpha):
        raise ValueError(f"{prefix}_neg_alpha must be finite, got {alpha!r}")
    return dist, alpha


def check_logq(logq, E):
    """The logQ correction of a sampled-softmax call: None, or fp32 [rows of E], contiguous, on E's device."""
    if logq is None:
        return None
    if not isinstance(logq, torch.Tensor) or logq.dtype != torch.float32 or tuple(logq.shape) != (E.shape[0],) \
            or not logq.is_contiguous() or logq.device != E.device:
        raise ValueError(f"logq must be a contiguous fp32 tensor of shape ({E.shape[0]},) on {E.device}")
    return logq


def site_salt(base, site):
    """Distinct 64-bit dropout salt per (model instance, dropout site)."""
    return (int(base) * 0x100000001B3 + 0x9E3779B97F4A7C15 * (site + 1)) & 0xFFFFFFFFFFFFFFFF


class Workspace:
    """Per-shape scratch buffers reused across steps (the C ABI allocates nothing)."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, name, shape, dtype):
        shape = tuple(int(s) for s in shape)
        t = self.bufs.get(name)
        if t is None or t.dtype != dtype or tuple(t.shape) != shape:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self.bufs[name] = t
        return t


# Events created while a stream is capturing a HIP graph are kept alive until that capture has ended
# (FusedTrainStep._capture_graphs releases them after instantiation): a per-step event dropped mid-capture -- the
# next unrolled step replacing it, a local going out of scope -- is otherwise destroyed while the capture still tracks
# it as a dependency source.
_CAPTURE_EVENTS = []


def capture_event():
    """torch.cuda.Event() for a fork / join inside a step; held until the end of the capture when one is running."""
    ev = torch.cuda.Event()
    if torch.cuda.is_current_stream_capturing():
        _CAPTURE_EVENTS.append(ev)
    return ev


def release_capture_events():
    _CAPTURE_EVENTS.clear()


def new_stream(device, avoid=()):
    """A torch.cuda.Stream whose handle differs from every stream in ``avoid`` and from the current stream.  torch
    deals its streams round-robin from a pool of 32 per priority, so in a long process a fresh draw can be a stream
    already in use -- the one being captured, say, which turns every fork onto it into a self-wait and the graph
    into one chain.  Re-drawn until distinct; RuntimeError after 32 draws."""
    taken = {s.cuda_stream for s in avoid} | {torch.cuda.current_stream(device).cuda_stream}
    for _ in range(32):
        s = torch.cuda.Stream(device=device)
        if s.cuda_stream not in taken:
            return s
    raise RuntimeError(f"no stream of torch's pool is free of the {len(taken)} to avoid")


class SideBranch:
    """One side stream and every fork onto it and join with it: the only place of a training step that touches
    events.  The engines run the work that needs only the batch's keys or a finished gradient here, beside the main
    chain (SASEngine.side, BERTEngine.side); FusedTrainStep runs the early optimizer updates on one of its own and
    warms up and captures on another.  Four rules hold that layout together:

    1. Event lifetime.  Every event is a capture_event(): one made while a stream is capturing outlives the
       capture (destroyed while the capture still tracks it, it crashed the process).
    2. Issue order.  A fork is RECORDED early (mark()) but its side work is ISSUED (run(after=mark)) only after the
       main stream's next launch: a captured graph keeps a node's first child on its queue, so the main chain then
       stays on the launch queue and the side branch takes the second.  Hence the after_first / after_rows
       callbacks and the grouped launch before the tail in SASEngine._backward_blocks_fused.  Measured the other way
       round: SAS cfg2, side branch first, 11 us of fork latency before rs_wgrad_grouped and 11 us of join latency
       before Adam; BERT cfg3, token index first, ~7 us before the embedding and ~12 us at the token gradient's
       queue hop (three interleaved rounds: 1.4145 / 1.4142 / 1.4149 -> 1.3983 / 1.4052 / 1.3978 ms/step).
    3. One writer per table.  All side work on one table goes to the SAME branch, so the table has one writer at a
       time in a fixed order (a SAS row head's table_grad or BERT sce_backward's head rows, then the lookup rows,
       joined once).
    4. Distinct streams.  The side stream is never the stream it forks from: new_stream() draws it apart from the
       streams given, and run() asserts it against the current one."""

    def __init__(self, device, avoid=()):
        self.stream = new_stream(device, avoid)
        self.end = None

    def mark(self):
        """A fork point: an event recorded on the current stream now."""
        ev = capture_event()
        ev.record()
        return ev

    @contextlib.contextmanager
    def run(self, after=None, end=True):
        """Issue the body on the side stream, ordered after the mark ``after`` (None: after the current stream's work
        so far).  On exit the branch's end event is recorded and kept in ``self.end``; end=False leaves a branch
        that a later run() continues before anyone joins it."""
        cur = torch.cuda.current_stream()
        assert self.stream.cuda_stream != cur.cuda_stream, "a side branch forked from its own stream"
        if after is not None:
            self.stream.wait_event(after)
        else:
            self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield self
            if end:
                self.end = capture_event()
                self.end.record()

    def join(self, ev=None):
        """The current stream waits for ``ev`` (default: the end of the branch's last run)."""
        torch.cuda.current_stream().wait_event(ev if ev is not None else self.end)
