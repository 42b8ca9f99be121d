"""Host restatement of the evaluation loader (rs_eval_negatives, rs_eval_batch, rbm_amd.metrics.evaluate).

Everything the kernels promise, written once in Python: the per-user raw draw stream (``draw`` in Python integers, as
include/recsys_hip.h writes it; ``draws_np`` the same in wrapping uint64 arithmetic), the alias rule, the stream filter
with its bound and fallback (``negatives_ref``), the rows of SASEvalDataset / BertEvalDataset in validation and test
mode (``rows_ref``, ``batches_ref``), the reference samplers' loop replayed on a given draw list (``reference_loop``)
and the equal-weight averaging of ``validate`` (``average_ref``).  tests/test_eval_loader_ref.py pins it to the
reference through tests/golden/eval_loader.npz (tools/gen_golden_eval.py).

The ``mistake=`` arguments plant one wrong reading each; they exist so that the CPU tests can show that the comparison
functions below (the ones the GPU tests use) reject it.
"""
import numpy as np

M64 = (1 << 64) - 1
A = 0xA0761D6478BD642F
C = 0x632BE59BD9B4E019
MAX_DRAWS = 4096          # rs_eval_negatives_max_draws()
NEGS_MAX = 1024           # rs_eval_negs_max()


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def user_key(seed, u):
    return splitmix64((seed ^ ((A * (u + 1)) & M64)) & M64)


def unpack_table(table):
    """(thr uint32 [V], alias int64 [V]) of a packed ItemProposal.table (int64 / uint64 [V])"""
    t = np.asarray(table).astype(np.int64).view(np.uint64)
    return (t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.int64)


def draw(seed, u, c, V, table=None, mistake=None):
    """x(u, c) in Python integers.  table: None (uniform over [1, V]) or (thr, alias)."""
    r = splitmix64((user_key(seed, u) + C * (c + 1)) & M64)
    if mistake == "zero_drawable":
        return (r * (V + 1)) >> 64
    prod = r * V
    s, frac = prod >> 64, (prod & M64) >> 32
    if table is None:
        return s + 1
    thr, alias = table
    return s + 1 if frac < int(thr[s]) else int(alias[s])


def draws_np(seed, u, c0, n, V, table=None, mistake=None):
    """x(u, c0 .. c0 + n) as int64, the same rule in wrapping uint64 arithmetic (V < 2^32)."""
    u64 = np.uint64
    with np.errstate(over="ignore"):
        z = u64(user_key(seed, u)) + u64(C) * np.arange(c0 + 1, c0 + n + 1, dtype=u64) + u64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        r = z ^ (z >> u64(31))
        W = V + 1 if mistake == "zero_drawable" else V
        mid = (r >> u64(32)) * u64(W) + (((r & u64(0xFFFFFFFF)) * u64(W)) >> u64(32))      # (r * W) >> 32
    s, frac = (mid >> u64(32)).astype(np.int64), (mid & u64(0xFFFFFFFF)).astype(np.uint32)
    if mistake == "zero_drawable":
        return s
    if table is None:
        return s + 1
    thr, alias = table
    return np.where(frac < thr[s], s + 1, alias[s])


def filter_stream(stream, seen, n_neg, V, max_draws=MAX_DRAWS, mistake=None):
    """(negs list, n_drawn) of one user: `stream(c0, n)` gives the raw draws c0 .. c0 + n.  Drops the items of
    `seen` (a set) and repeats of kept items, keeps the first n_neg in stream order; after max_draws raw draws the open
    slots take the smallest ids of [1, V] neither seen nor kept, ascending (n_drawn = -1 - slots filled that way)."""
    kept, have = [], set()
    for c0 in range(0, max_draws, 64):
        for j, v in enumerate(stream(c0, min(64, max_draws - c0))):
            v = int(v)
            if v in seen or (v in have and mistake != "keep_repeats"):
                continue
            kept.append(v)
            have.add(v)
            if len(kept) == n_neg:
                return kept, c0 + j + 1
    before = len(kept)
    for v in range(1, V + 1):
        if len(kept) == n_neg:
            break
        if v not in seen and v not in have:
            kept.append(v)
    filled = len(kept) - before
    kept += [0] * (n_neg - len(kept))
    return kept, -1 - filled


def seen_sets(train, val, test, mistake=None, max_len=None):
    """per user the whole history train + val + test (the planted mistake: the max_len window of train only)"""
    if mistake == "window_seen":
        return [set(map(int, list(tr)[-max_len:])) for tr in train]
    return [set(map(int, tr)) | {int(np.ravel(v)[0]), int(np.ravel(t)[0])} for tr, v, t in zip(train, val, test)]


def negatives_ref(seen, V, n_neg, seed, table=None, users=None, max_draws=MAX_DRAWS, mistake=None):
    """(negs int64 (n, n_neg), n_drawn int64 (n,)) of rs_eval_negatives for the users `users` (default: all)."""
    users = range(len(seen)) if users is None else users
    negs, drawn = [], []
    for u in users:
        k, d = filter_stream(lambda c0, n, u=u: draws_np(seed, u, c0, n, V, table, mistake), seen[u], n_neg, V,
                             max_draws, mistake)
        negs.append(k)
        drawn.append(d)
    return np.array(negs, np.int64).reshape(len(negs), n_neg), np.array(drawn, np.int64)


def reference_loop(draws, seen, n_neg):
    """RandomNegativeSampler.generate_negative_samples' inner loops (negative_samplers/random.py:28-33) for one user,
    with `np.random.choice(item_count) + 1` read from the list `draws`.  Raises StopIteration if the list runs out."""
    it = iter(int(x) for x in draws)
    samples = []
    for _ in range(n_neg):
        item = next(it)
        while item in seen or item in samples:
            item = next(it)
        samples.append(item)
    return samples


def rows_ref(train, val, test, negs, T, mode, model_code, V, mistake=None):
    """(seq (n, T), cand (n, 1 + n_neg), labels) int64: SASEvalDataset / BertEvalDataset.__getitem__ for every user,
    with _get_eval_dataset's history (train, + the validation item in test mode)."""
    n = len(train)
    negs = np.asarray(negs, np.int64)
    seq = np.zeros((n, T), np.int64)
    cand = np.zeros((n, 1 + negs.shape[1]), np.int64)
    labels = np.zeros_like(cand)
    for u in range(n):
        h = [int(x) for x in train[u]]
        v, t = int(np.ravel(val[u])[0]), int(np.ravel(test[u])[0])
        if mode == "test" and mistake != "test_without_val":
            h = h + [v]
        if model_code == "bert":
            # the planted mistake: a full window leaves no room for [MASK], which then overwrites the last item
            h = (h[-T:][:T - 1] + [V + 1]) if mistake == "truncate_before_mask" else h + [V + 1]
        h = h[-T:]
        seq[u, T - len(h):] = h
        ans = t if mode == "test" else v
        if mistake == "answer_last":
            cand[u] = list(negs[u]) + [ans]
            labels[u, -1] = 1
        else:
            cand[u] = [ans] + list(negs[u])
            labels[u, 0] = 1
    return seq, cand, labels


def batches_ref(rows, batch_size, mistake=None):
    """the DataLoader(shuffle=False) batches of the rows: users in order, the last batch partial"""
    n = rows[0].shape[0]
    out = [tuple(a[i:i + batch_size] for a in rows) for i in range(0, n, batch_size)]
    if mistake == "drop_partial" and n % batch_size:
        out = out[:-1]
    return out


def average_ref(batch_metrics, sizes=None, mistake=None):
    """AverageMeterSet's average over the batches' metric dicts: every batch has weight one"""
    keys = list(batch_metrics[0])
    if mistake == "weight_by_size":
        w = np.asarray(sizes, np.float64)
        return {k: float(np.dot(w, [m[k] for m in batch_metrics]) / w.sum()) for k in keys}
    return {k: float(np.mean(np.array([m[k] for m in batch_metrics], np.float64))) for k in keys}


# ---------------------------------------------------------------- the comparisons (CPU and GPU tests alike)
def check_negatives(negs, n_drawn, ref_negs, ref_drawn):
    negs, ref_negs = np.asarray(negs, np.int64), np.asarray(ref_negs, np.int64)
    assert negs.shape == ref_negs.shape, (negs.shape, ref_negs.shape)
    bad = np.nonzero((negs != ref_negs).any(axis=1))[0]
    assert bad.size == 0, f"negatives differ for users {bad[:8].tolist()} ({bad.size} in all)"
    if n_drawn is not None:
        d, r = np.asarray(n_drawn, np.int64), np.asarray(ref_drawn, np.int64)
        assert np.array_equal(d, r), f"n_drawn differs for users {np.nonzero(d != r)[0][:8].tolist()}"


def check_properties(negs, seen, V):
    """ids in [1, V], distinct per user, disjoint from seen(u)"""
    negs = np.asarray(negs, np.int64)
    assert negs.min() >= 1 and negs.max() <= V, (int(negs.min()), int(negs.max()))
    for u, row in enumerate(negs):
        assert len(set(row.tolist())) == row.size, f"user {u}: a repeated negative"
        assert not (set(row.tolist()) & seen[u]), f"user {u}: a seen item among the negatives"


def check_batches(got, want):
    assert len(got) == len(want), f"{len(got)} batches, expected {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("seq", "candidates", "labels"), g, w):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape, (i, name, a.shape, b.shape)
            assert np.array_equal(a, b), f"batch {i}: {name} differs in rows {np.nonzero((a != b).any(axis=1))[0][:8]}"


def check_average(got, want, tol=1e-9):
    assert list(got) == list(want), (list(got), list(want))
    for k in want:
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


# ---------------------------------------------------------------- shared test data
def make_users(rng, n, V, lo, hi, zipf=False):
    """(train, val, test): n users with lo .. hi training items (ids with repeats, as real histories have)"""
    train, val, test = [], [], []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        if zipf:
            w = 1.0 / np.arange(1, V + 1)
            h = rng.choice(np.arange(1, V + 1), size=L + 2, p=w / w.sum())
        else:
            h = rng.integers(1, V + 1, size=L + 2)
        train.append([int(x) for x in h[:-2]])
        val.append([int(h[-2])])
        test.append([int(h[-1])])
    return train, val, test
