#!/usr/bin/env python
"""Times full-catalogue top-K (K = 10) and full-rank against what the same tree could do before (GPU only).

    python tools/fullrank_bench.py [--reps 50] [--out profiles/fullrank_bench.json] [--shapes V:d,...] [--B 64,1024]

Per shape (V items + the padding row, d, B; bf16) one JSON line: the median over --reps graph replays, each timed by
its own pair of HIP events, of
  * ops.full_topk (K = 10) and ops.full_rank (no exclusion list, a bias), and
  * the baseline: ops.linear_fwd into a (B, V + 1) fp32 score buffer followed by torch.topk (skipped when the buffer
    does not fit),
with the rates the times amount to -- 2 B V d flop over the time, and E's bytes over the time -- and the E-streaming
floor (E's bytes over the HBM bandwidth, 8 TB/s peak and the 6.3 TB/s a plain copy reaches).  No pass / fail.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rbm_amd  # noqa: E402,F401
from rbm_amd import ops  # noqa: E402

SHAPES = [(3416, 128), (54542, 128), (1000000, 256)]
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12


def median_us(fn, reps, warmup=5):
    """Median of `reps` replays of fn captured as one graph, each between its own pair of events."""
    fn()                                   # first use outside the capture (kernel attributes, allocator)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()                        # (outputs stay alive with the graph)
    for _ in range(warmup):
        g.replay()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        g.replay()
        b.record()
    torch.cuda.synchronize()
    del keep
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default=",".join(f"{v}:{d}" for v, d in SHAPES))
    ap.add_argument("--B", default="64,1024")
    ap.add_argument("--K", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fullrank_bench needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = []
    for V, d in (tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")):
        V1 = V + 1
        E = (0.05 * torch.randn(V1, d, device="cuda", generator=gen)).bfloat16()
        bias = 0.01 * torch.randn(V1, device="cuda", generator=gen)
        for B in (int(x) for x in a.B.split(",")):
            h = torch.randn(B, d, device="cuda", generator=gen).bfloat16()
            tgt = torch.randint(1, V1, (B,), device="cuda", generator=gen)
            flop, ebytes = 2.0 * B * V * d, 2.0 * V * d
            r = {"V": V, "d": d, "B": B, "K": a.K, "dtype": "bf16", "reps": a.reps}
            t_topk = median_us(lambda: ops.full_topk(h, E, a.K, bias=bias), a.reps)
            t_rank = median_us(lambda: ops.full_rank(h, E, tgt, bias=bias, check=False), a.reps)
            for name, t in (("topk", t_topk), ("rank", t_rank)):
                r[f"{name}_us"] = round(t, 2)
                r[f"{name}_tflops"] = round(flop / t / 1e6, 2)
                r[f"{name}_E_GBps"] = round(ebytes / t / 1e3, 1)
            try:
                S = torch.empty((B, V1), dtype=torch.float32, device="cuda")

                def dense():
                    ops.linear_fwd(h, E, S, bias=bias)
                    return torch.topk(S[:, 1:], a.K, dim=1)
                r["baseline_linear_fwd_topk_us"] = round(median_us(dense, a.reps), 2)
                r["baseline_linear_fwd_us"] = round(median_us(lambda: ops.linear_fwd(h, E, S, bias=bias), a.reps), 2)
                r["baseline_score_bytes"] = B * V1 * 4
                del S
            except torch.cuda.OutOfMemoryError:
                r["baseline_linear_fwd_topk_us"] = None
            r["ws_bytes"] = int(ops.full_ws(h, 1, V1, a.K).numel())
            r["floor_us_hbm_8.0TBps"] = round(ebytes / HBM_PEAK * 1e6, 2)
            r["floor_us_hbm_6.3TBps"] = round(ebytes / HBM_COPY * 1e6, 2)
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
