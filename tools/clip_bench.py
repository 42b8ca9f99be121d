#!/usr/bin/env python
"""Times whole steps with max_grad_norm = None / inf / a value that clips, and the norm's launches alone (GPU only).

    python tools/clip_bench.py [--reps 30] [--rounds 3] [--out profiles/clip_bench.json]
                               [--shapes sas_cfg2,bert_cfg5,bert_cfg5_sce_dense,bert_cfg5_sce_sparse] [--k 4096]
                               [--order none,inf,clip]

Per shape three bf16 step objects of one process, captured, then graph replays (median over --reps replays, each
between its own pair of HIP events) in --rounds interleaved rounds; one JSON line per shape:
  * "step_ms": every round's median per variant; "none" runs exactly the launches of a step built without the argument.
    "clip" gets a hundredth of the norm the "inf" twin measured on its last warm-up step, so it clips on every replay
    although the replays train on one batch ("coef": the last timed replay's coefficient).  A step object's place in the process moves its time by a few percent at the 1M-item shapes
    (tools/sgd_bench.py), so differences of that size between the variants say nothing.
  * "norm_us": the norm's launches alone (rs_gradnorm_dense [+ rs_gradnorm_rows per table] + rs_gradnorm_finish, the
    step's own call replayed as one graph), "norm_elems" the gradient elements they cover by the layout (sparse
    tables: list capacity x row width, an upper bound of the touched rows) and "norm_tbs" = 4 * norm_elems / time:
    to set beside tools/diag/hbm_bw.py's read figure.  The kernels' own times come from a separate
    rocprofv3 --kernel-trace --stats run of this tool.
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
from rbm_amd.train_step import FusedTrainStep  # noqa: E402
import bert_sce_bench as bb  # noqa: E402
import sas_ce_bench as sb  # noqa: E402
from sas_ce_bench import launch_us, replay_us  # noqa: E402
from sgd_bench import make_batch  # noqa: E402


def shapes():
    c2, c5 = sb.CONFIGS["cfg2"], bb.CONFIGS["cfg5"]
    return {"sas_cfg2": ("sas", c2, "bce", "dense"), "bert_cfg5": ("bert", c5, None, "dense"),
            "bert_cfg5_sce_dense": ("bert", c5, "sampled_ce", "dense"),
            "bert_cfg5_sce_sparse": ("bert", c5, "sampled_ce", "sparse")}


def norm_spec(t):
    """the step's `sparse` argument from the lists its last step built (no branch to join here)"""
    if t._sparse_tables is None:
        return None
    return [(lo, rows, d, lst, cnt) for (_, tabs), (lst, cnt, _) in zip(t._sparse_tables, t._sparse_bufs)
            for lo, rows, d in tabs]


def whole_step(kind, cfg, loss, table_optim, K, reps, rounds, order):
    batch = make_batch(kind, cfg, np.random.default_rng(0))
    if loss == "sampled_ce":
        batch.append(torch.from_numpy(np.random.default_rng(1).integers(1, cfg["V"] + 1, K)).cuda())
    make = bb.model if kind == "bert" else sb.model
    kw = dict(max_labelled=cfg["cap"]) if kind == "bert" else {}
    steps = {}
    for name in order:                           # built, and replayed within a round, in this order
        c = None if name == "none" else float("inf")
        steps[name] = FusedTrainStep(make(cfg), lr=1e-3, loss=loss, table_optim=table_optim, max_grad_norm=c,
                                     **kw).capture(*batch, warmup=3)
    torch.cuda.synchronize()
    norm = float(steps["inf"].grad_norm)
    steps["clip"].set_max_grad_norm(0.01 * norm)
    ms = {k: [] for k in steps}
    for _ in range(rounds):                      # interleaved rounds
        for k, t in steps.items():
            ms[k].append(round(replay_us(t.g_compute, reps) / 1e3, 4))
    med = {k: statistics.median(x) for k, x in ms.items()}
    t = steps["clip"]
    torch.cuda.synchronize()
    coef = float(t.clip_coef)                    # of the last timed replay (below, the norm runs on a cleared gradient)
    spec = norm_spec(t)
    us = [launch_us(lambda: t._clip_norm(spec), reps) for _ in range(rounds)]
    if spec:
        elems = sum(hi - lo for lo, hi, _ in t.opt._sparse_segments(spec)) + sum(lst.numel() * d
                                                                                  for _, _, d, lst, _ in spec)
    else:
        elems = t.flat.numel
    return {"step_ms": ms, "inf_over_none": round(med["inf"] / med["none"], 4),
            "clip_over_none": round(med["clip"] / med["none"], 4), "grad_norm": norm,
            "coef": coef, "params": t.flat.numel, "norm_us": us, "norm_elems": elems,
            "norm_partials": t._clip_ws.numel(),
            "norm_tbs": round(4 * elems / (statistics.median(us) * 1e-6) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--order", default="none,inf,clip", help="the order the three step objects are built in")
    ap.add_argument("--shapes", default="sas_cfg2,bert_cfg5,bert_cfg5_sce_dense,bert_cfg5_sce_sparse")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "clip_bench needs a GPU"
    lines = []
    table = shapes()
    order = a.order.split(",")
    assert sorted(order) == ["clip", "inf", "none"], a.order
    for name in [x for x in a.shapes.split(",") if x]:
        kind, cfg, loss, topt = table[name]
        r = {"shape": name, "loss": loss or ("ce" if kind == "bert" else "bce"), "table_optim": topt,
             **{k: cfg[k] for k in ("B", "T", "V", "d", "L")}, "dtype": "bf16", "reps": a.reps, "rounds": a.rounds,
             "order": a.order,
             **({"K": a.k} if loss == "sampled_ce" else {}),
             **whole_step(kind, cfg, loss, topt, a.k, a.reps, a.rounds, order)}
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        if a.out:                     # written as it grows: a long run leaves what it finished
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
