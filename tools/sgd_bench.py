#!/usr/bin/env python
"""Times the fused SGD sweep against the Adam sweep, and whole steps with optimizer="sgd" beside "adam" (GPU only).

    python tools/sgd_bench.py [--reps 30] [--rounds 3] [--out profiles/sgd_bench.json]
                              [--sizes 662019,268435456] [--shapes sas_cfg2,bert_cfg5]

Graph replays (median over --reps replays, each between its own pair of HIP events), --rounds interleaved rounds, one
JSON line per measurement:
  * "sweep": rs_sgd_step (momentum 0.9: p, g, buf; momentum 0: p, g) and the Adam sweep (rs_adam_prepare_step, the
    step's first-range launch, and rs_adam_step) on the SAME p / g / bf16 buffers in one process, with the bf16 copy,
    zero_grad on.  The gradient is zero from the second replay on (the sweep cleared it), so neither kernel stores
    it: "bytes_per_elem" counts from the code p 4 + 4, g 4, bf16 2, and 8 per moment / momentum buffer -- SGD 22
    (14 without momentum), Adam 30 (each 4 more on a step whose gradient is non-zero everywhere).  "tbs" = bytes moved
    / median time.
  * "step": bf16 steps of sas_cfg2 (bce) and bert_cfg5 (full cross-entropy, 1M items) with the two optimizers as two
    step objects of one process: "step_ms", the optimizer's launches alone ("opt_us", FusedTrainStep._update
    replayed as one graph: under Adam at bert_cfg5 that is the whole update at the end of the step, not the early
    head / token split the step itself uses) and their share.  A step object's place in the process moves its
    time by a few percent at the 1M-item shape, so differences of that size between the two say nothing.
No pass / fail.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rbm_amd  # noqa: E402,F401
import rbm_amd.data as synth  # noqa: E402
from rbm_amd import ops  # noqa: E402
from rbm_amd.train_step import FusedTrainStep  # noqa: E402
import bert_sce_bench as bb  # noqa: E402
import sas_ce_bench as sb  # noqa: E402
from sas_ce_bench import launch_us, replay_us  # noqa: E402

BYTES = {"sgd_momentum": 22, "sgd_plain": 14, "adam_prepare_step": 30, "adam_step": 30}


def sweep(n, reps, rounds):
    dev = "cuda"
    g0 = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, generator=g0, device=dev)
    g = torch.zeros(n, device=dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)     # m doubles as the momentum buffer
    pb = torch.empty(n, dtype=torch.bfloat16, device=dev)
    st_a = torch.zeros(144, dtype=torch.float64, device=dev)
    st_s = torch.zeros(8, dtype=torch.float64, device=dev)
    hy_a = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.0], dtype=torch.float64, device=dev)
    hy_s = torch.tensor([1e-3, 0.9, 0.0], dtype=torch.float64, device=dev)
    fns = {
        "sgd_momentum": lambda: ops.sgd_step(p, g, m, pb, st_s, hy_s, zero_grad=True, prepare=True),
        "sgd_plain": lambda: ops.sgd_step(p, g, None, pb, st_s, hy_s, zero_grad=True, prepare=True),
        "adam_prepare_step": lambda: ops.adam_prepare_step(p, g, m, v, pb, st_a, hy_a, zero_grad=True),
        "adam_step": lambda: ops.adam_step(p, g, m, v, pb, st_a, hy_a, zero_grad=True),
    }
    graphs = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            fn()
    us = {k: [] for k in fns}
    for _ in range(rounds):                      # interleaved rounds
        for k, gr in graphs.items():
            us[k].append(round(replay_us(gr, reps), 2))
    med = {k: statistics.median(x) for k, x in us.items()}
    return {"us": us, "median_us": med, "bytes_per_elem": BYTES,
            "tbs": {k: round(BYTES[k] * n / (med[k] * 1e-6) / 1e12, 3) for k in fns},
            "sgd_momentum_over_adam_prepare_step": round(med["sgd_momentum"] / med["adam_prepare_step"], 3)}


def shapes():
    return {"sas_cfg2": ("sas", sb.CONFIGS["cfg2"], "bce"), "bert_cfg5": ("bert", bb.CONFIGS["cfg5"], None)}


def make_batch(kind, cfg, rng):
    zipf = synth.ZipfItems(cfg["V"])
    if kind == "bert":
        b = synth.bert_batch(rng, cfg["B"], cfg["T"], cfg["V"], mask_prob=cfg["mask"], shape=cfg["shape"], zipf=zipf)
    else:
        b = synth.sas_batch(rng, cfg["B"], cfg["T"], cfg["V"], shape=cfg["shape"], zipf=zipf)
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in b]


def whole_step(kind, cfg, loss, reps, rounds):
    batch = make_batch(kind, cfg, np.random.default_rng(0))
    make = bb.model if kind == "bert" else sb.model
    kw = dict(max_labelled=cfg["cap"]) if kind == "bert" else {}
    opts = {"adam": {}, "sgd": dict(optimizer="sgd", momentum=0.9)}
    steps = {k: FusedTrainStep(make(cfg), lr=1e-3, loss=loss, **kw, **o).capture(*batch, warmup=3)
             for k, o in opts.items()}
    ms = {k: [] for k in steps}
    for _ in range(rounds):                      # interleaved rounds
        for k, t in steps.items():
            ms[k].append(round(replay_us(t.g_compute, reps) / 1e3, 4))
    med = {k: statistics.median(x) for k, x in ms.items()}
    r = {"step_ms": ms, "sgd_over_adam": round(med["sgd"] / med["adam"], 3), "opt_us": {}, "opt_share": {},
         "params": steps["adam"].flat.numel}
    for k, t in steps.items():
        us = [launch_us(t._update, reps) for _ in range(rounds)]
        r["opt_us"][k] = us
        r["opt_share"][k] = round(statistics.median(us) / 1e3 / med[k], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="662019,268435456")
    ap.add_argument("--shapes", default="sas_cfg2,bert_cfg5")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sgd_bench needs a GPU"
    lines = []

    def emit(r):
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        if a.out:                     # written as it grows: a long run leaves what it finished
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    for n in [int(x) for x in a.sizes.split(",") if x]:
        emit({"kind": "sweep", "n": n, "reps": a.reps, "rounds": a.rounds, **sweep(n, a.reps, a.rounds)})
    table = shapes()
    for name in [x for x in a.shapes.split(",") if x]:
        kind, cfg, loss = table[name]
        emit({"kind": "step", "shape": name, "loss": loss or "ce", **{k: cfg[k] for k in ("B", "T", "V", "d", "L")},
              "dtype": "bf16", "reps": a.reps, "rounds": a.rounds, **whole_step(kind, cfg, loss, a.reps, a.rounds)})


if __name__ == "__main__":
    main()
