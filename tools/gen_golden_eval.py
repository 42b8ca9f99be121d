"""Golden vectors for tests/eval_loader_ref.py from the REFERENCE's evaluation pipeline (container-only).

Runs the reference's ``RandomNegativeSampler.generate_negative_samples`` (``BS/dataloaders/negative_samplers/
random.py``) with ``np.random.choice`` fed from a recorded per-user draw list -- the raw stream x(u, c) of
tests/eval_loader_ref.py -- and its ``SASEvalDataset`` / ``BertEvalDataset`` (``BS/dataloaders/sas.py:125-153``,
``bert.py:116-142``) on the histories ``_get_eval_dataset`` hands them in validation and test mode, and writes
``tests/golden/eval_loader.npz``: the histories, the draw lists, the reference's negatives and its dataset rows (data
only).  ``tests/test_eval_loader_ref.py`` must reproduce them with the restatement -- the pin of what the GPU tests
compare against.

The reference never travels to the GPU box; this script refuses to run when ``/root/reference`` is absent and
writes nothing into the reference tree (no bytecode, temp CWD).

    python tools/gen_golden_eval.py
"""
import os
import sys
import tempfile
import types
from copy import deepcopy

sys.dont_write_bytecode = True
REF = "/root/reference/NerualNetwork/bert4rec&sas4rec"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "eval_loader.npz")

if not os.path.isdir(REF):
    raise SystemExit("gen_golden_eval: /root/reference is absent; fixtures are generated in the build container")

import numpy as np  # noqa: E402

_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = object
sys.modules["torch.utils.tensorboard"] = _tb
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.chdir(tempfile.mkdtemp())

import dataloaders.negative_samplers.random as ref_random  # noqa: E402  (reference)
from dataloaders.sas import SASEvalDataset  # noqa: E402  (reference)
from dataloaders.bert import BertEvalDataset  # noqa: E402  (reference)
import eval_loader_ref as R  # noqa: E402  (this repo: the restatement whose stream is recorded)

U, V, N_NEG, T, SEED, N_DRAWS = 37, 150, 40, 12, 2024, 512


def histories():
    rng = np.random.default_rng(7)
    # at least two training items: the reference's sampler reads train[user][1] (random.py:19)
    lens = [2, 3, T - 2, T - 1, T, T + 1, T + 5, 60] + [int(x) for x in rng.integers(2, 61, size=U - 8)]
    train = [[int(x) for x in rng.integers(1, V + 1, size=n)] for n in lens]
    val = [[int(rng.integers(1, V + 1))] for _ in lens]
    test = [[int(rng.integers(1, V + 1))] for _ in lens]
    return train, val, test


def reference_negatives(train, val, test, draws):
    """the reference's sampler; np.random.choice(item_count) returns the current user's next recorded draw - 1"""
    state = {"user": None, "c": 0}
    used = np.zeros(U, np.int64)

    def users(a, b):
        for u in range(a, b):
            state["user"], state["c"] = u, 0
            yield u

    def choice(n):
        assert n == V
        u, c = state["user"], state["c"]
        state["c"] = c + 1
        used[u] = c + 1
        return int(draws[u, c]) - 1

    real_choice, real_trange = np.random.choice, ref_random.trange
    np.random.choice, ref_random.trange = choice, users
    try:
        s = ref_random.RandomNegativeSampler(train, val, test, U, V, N_NEG, SEED, ".", "golden")
        out = s.generate_negative_samples()
    finally:
        np.random.choice, ref_random.trange = real_choice, real_trange
    return np.array([out[u] for u in range(U)], np.int64), used


def dataset_rows(train, val, test, negs, mode, model_code):
    answers = val if mode == "val" else test
    u2seq = deepcopy(train)                       # _get_eval_dataset (sas.py:51-61, bert.py:49-61)
    if mode == "test":
        for u, seq in enumerate(u2seq):
            seq.append(val[u][0])
    neg = {u: [int(x) for x in negs[u]] for u in range(U)}
    ds = SASEvalDataset(u2seq, answers, T, neg) if model_code == "sas" else BertEvalDataset(u2seq, answers, T, V + 1,
                                                                                            neg)
    rows = [ds[u] for u in range(len(ds))]
    return tuple(np.stack([np.asarray(r[k], dtype=np.int64) for r in rows]) for k in range(3))


def main():
    train, val, test = histories()
    draws = np.stack([R.draws_np(SEED, u, 0, N_DRAWS, V) for u in range(U)]).astype(np.int32)
    negs, used = reference_negatives(train, val, test, draws)
    off = np.zeros(U + 1, np.int64)
    off[1:] = np.cumsum([len(h) for h in train])
    out = {"U": np.int64(U), "V": np.int64(V), "n_neg": np.int64(N_NEG), "T": np.int64(T), "seed": np.int64(SEED),
           "train_off": off, "train_items": np.array([i for h in train for i in h], np.int64),
           "val": np.array([v[0] for v in val], np.int64), "test": np.array([t[0] for t in test], np.int64),
           "draws": draws, "negs": negs, "n_drawn": used}
    for model_code in ("sas", "bert"):
        for mode in ("val", "test"):
            seq, cand, labels = dataset_rows(train, val, test, negs, mode, model_code)
            out.update({f"{model_code}_{mode}/seq": seq, f"{model_code}_{mode}/cand": cand,
                        f"{model_code}_{mode}/labels": labels})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; draws used per user", used.min(), "..", used.max())


if __name__ == "__main__":
    main()
