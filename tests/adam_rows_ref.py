"""Reference for the sparse (touched-rows-only) Adam of a table (rs_adam_rows, FusedAdam.step(sparse=...)).

The rule, per step t (ONE global step count, advanced once per step) with touched set S_t:
  r in S_t    : every element of row r takes the dense sweep's update (csrc/adam_math.h, restated below element by
                element), the bf16 copy of the row is rewritten, the row's gradient is cleared;
  r not in S_t: p / m / v / bf16 of row r keep their bits; the row's gradient is neither read nor written.

`update` restates adam_elem_update with the step's scalars cast to float exactly where adam_math.h casts them
(the hyperparameters are doubles; bias corrections formed in double):
    gj    = g * gs                      (gs = 1: g itself)
    m     = fma(1 - b1, gj - m, m)
    v     = fma((1 - b2) * gj, gj, v * b2)
    denom = sqrt(v) / sqrt(bc2) + eps
    p     = fma(-lr / bc1, m / denom, p)
in float64 (the reference: no rounding but the scalars') or in an emulation of the kernel's float32 (every
operation rounded to float32, a fused multiply-add rounded once).  Against torch.optim.SparseAdam the rule differs
only in where eps sits: SparseAdam takes denom = sqrt(v) + eps and step size lr * sqrt(bc2) / bc1.

The checks (`check_state`, `check_untouched`) are the ones the GPU tests apply to the kernel: v within 4 float32
ulps per element, m and p within 4 ulps of the tensor's largest magnitude (the bars tests/test_adam_gpu.py holds
the dense sweep to), the bf16 copy the exact rounding of p, the gradient of touched rows cleared, untouched rows bit
for bit.  MISTAKES names the planted errors the CPU test proves these checks reject.
"""
import math

import numpy as np

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
ULPS = 4.0

# the GPU test's 300-step case (tests/test_adam_rows_gpu.py): R = 1000 rows of 64, 10 fresh ids (+ duplicates) per
# step, so a row takes about 3 updates and at most about 10 -- the update counts the dense bar was set at (5 steps in
# tests/test_adam_gpu.py); each update adds at most ~1 ulp to v (two roundings of half an ulp: v * b2 and the fma)
LONG = dict(seed=11, R=1000, d=64, steps=300, per_step=10)

MISTAKES = ("decay_untouched", "twice", "per_row_step", "eps_sparse_adam", "no_clear", "stale_bf16")


def bf16_round(x):
    """float32 array -> the float32 value of its bf16 rounding (round to nearest even; finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def step_scalars(t, hyper, divisor=None):
    """adam_scalars + adam_elem of step t: hyper = (lr, beta1, beta2, eps, weight_decay) as Python floats."""
    lr, b1, b2, eps, wd = (float(x) for x in hyper)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    gs = F32(1.0) / F32(divisor) if divisor is not None else F32(1.0)
    return dict(step_size=F32(lr / bc1), bc2s=F32(math.sqrt(bc2)), gs=gs, b2=F32(b2), omb1=F32(1.0 - b1),
                omb2=F32(1.0 - b2), eps=F32(eps), wd=F32(wd))


def _fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64; one rounding of the float64 sum
    (itself rounded: a double rounding in rare ties, far below the checks' 4 ulps)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def update(P, G, M, V, s, dtype=np.float64, eps_sparse_adam=False):
    """One adam_elem_update on arrays; dtype float64 = the reference, float32 = the kernel's arithmetic emulated.
    Returns (P, M, V).  eps_sparse_adam: the planted SparseAdam form of the denominator."""
    k = {n: np.asarray(x, dtype=dtype) for n, x in s.items()}
    P, G, M, V = (np.asarray(x, dtype=dtype) for x in (P, G, M, V))
    f32 = dtype == np.float32
    fma = _fma32 if f32 else (lambda a, b, c: a * b + c)
    gj = G if float(s["gs"]) == 1.0 else G * k["gs"]
    if float(s["wd"]) != 0.0:
        gj = fma(k["wd"], P, gj)
    M = fma(k["omb1"], gj - M, M)
    V = fma(k["omb2"] * gj, gj, V * k["b2"])
    if eps_sparse_adam:
        denom = np.sqrt(V) + k["eps"]
        P = fma(-(k["step_size"] * k["bc2s"]), M / denom, P)
    else:
        denom = np.sqrt(V) / k["bc2s"] + k["eps"]
        P = fma(-k["step_size"], M / denom, P)
    return P, M, V


class Table:
    """p / g / m / v [R][d] in `dtype` and the bf16 copy of p (held as its float32 value)."""

    def __init__(self, p, g, m, v, dtype=np.float64):
        self.dtype = dtype
        self.p, self.g, self.m, self.v = (np.array(x, dtype=dtype).reshape(np.shape(p)) for x in (p, g, m, v))
        self.bf16 = bf16_round(np.asarray(p, dtype=np.float32))
        self.row_steps = np.zeros(self.p.shape[0], dtype=np.int64)     # only the per_row_step mistake reads it

    def copy(self):
        t = Table(self.p, self.g, self.m, self.v, self.dtype)
        t.bf16 = self.bf16.copy()
        t.row_steps = self.row_steps.copy()
        return t


def sparse_step(tab, lists, t, hyper, zero_grad=True, mistake=None):
    """Step t on `tab` in place: lists = one or more id arrays (the key arrays of the step; ids of 0 or outside the
    table are dropped, an id named twice -- in one list or in two -- is updated ONCE).  Returns the sorted touched
    rows.  mistake: one of MISTAKES, planted."""
    R = tab.p.shape[0]
    ids = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]) if len(lists) else \
        np.zeros(0, np.int64)
    ids = ids[(ids >= 1) & (ids < R)]
    rows = np.unique(ids)
    todo = [rows]
    if mistake == "twice":          # every further occurrence of an id updates its row again
        rest = ids
        todo = []
        while rest.size:
            u, first = np.unique(rest, return_index=True)
            todo.append(u)
            rest = np.delete(rest, first)
    s = step_scalars(t, hyper)
    for rs in todo:
        if mistake == "per_row_step":
            tab.row_steps[rs] += 1
            for r in rs:
                sr = step_scalars(int(tab.row_steps[r]), hyper)
                tab.p[r], tab.m[r], tab.v[r] = update(tab.p[r], tab.g[r], tab.m[r], tab.v[r], sr, tab.dtype)
        else:
            tab.p[rs], tab.m[rs], tab.v[rs] = update(tab.p[rs], tab.g[rs], tab.m[rs], tab.v[rs], s, tab.dtype,
                                                     eps_sparse_adam=mistake == "eps_sparse_adam")
    if mistake == "decay_untouched":    # the dense rule on a row without a gradient
        rest = np.setdiff1d(np.arange(R), rows)
        z = np.zeros_like(tab.p[rest])
        tab.p[rest], tab.m[rest], tab.v[rest] = update(tab.p[rest], z, tab.m[rest], tab.v[rest], s, tab.dtype)
    if mistake != "stale_bf16":
        tab.bf16[rows] = bf16_round(tab.p[rows].astype(np.float32))
    if zero_grad and mistake != "no_clear":
        tab.g[rows] = 0
    return rows


# ------------------------------------------------------------------ the checks
def ulps_each(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / EPS32 / np.maximum(np.abs(b), 1e-30)).max()) if a.size else 0.0


def ulps_of_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / EPS32 / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def state_errors(got, ref):
    """{name: figure} of a float32 state `got` (anything with p / m / v / bf16 arrays) against the float64 `ref`."""
    return {"v": ulps_each(got.v, ref.v), "m": ulps_of_max(got.m, ref.m), "p": ulps_of_max(got.p, ref.p)}


def check_state(got, ref, cleared_rows=None):
    """The problems (a list of strings, empty when it passes) of `got` against the float64 reference: the three
    bounds, the bf16 copy = the rounding of got's own p bit for bit, the gradient of cleared_rows zero."""
    bad = [f"{k}: {e:.3g} ulps > {ULPS}" for k, e in state_errors(got, ref).items() if not e <= ULPS]
    if not same_bits(got.bf16, bf16_round(np.asarray(got.p, np.float32))):
        bad.append("bf16 copy is not the rounding of p")
    if cleared_rows is not None and np.count_nonzero(np.asarray(got.g)[cleared_rows]):
        bad.append("gradient of a touched row not cleared")
    return bad


def check_untouched(before, after, rows):
    """Problems with the rows outside `rows`: p / m / v / bf16 / g must keep their bits (NaN gradients included)."""
    R = np.asarray(before.p).shape[0]
    rest = np.setdiff1d(np.arange(R), np.asarray(rows, dtype=np.int64))
    return [f"untouched rows changed in {n}" for n in ("p", "m", "v", "bf16", "g")
            if not same_bits(np.asarray(getattr(before, n))[rest], np.asarray(getattr(after, n))[rest])]


def scenario(seed, R, d, steps, per_step, tiny_cols=0, lists=1):
    """Deterministic test data: initial (p, m, v) and, per step, `lists` id arrays (fresh random touched sets with
    duplicates, zeros and out-of-range ids among them), the gradient rows for the touched ids and a learning rate
    that changes every step.  tiny_cols: that many leading columns carry gradients and second moments near eps^2,
    where the place of eps in the denominator decides the update."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((R, d)).astype(np.float32)
    m = (0.1 * rng.standard_normal((R, d))).astype(np.float32)
    v = (0.01 * rng.standard_normal((R, d)) ** 2 + 1e-6).astype(np.float32)
    if tiny_cols:
        m[:, :tiny_cols] *= 1e-7
        v[:, :tiny_cols] = (1e-16 * rng.random((R, tiny_cols))).astype(np.float32)
    out = []
    for t in range(1, steps + 1):
        ls = []
        for _ in range(lists):
            ids = rng.integers(1, max(R, 2), size=per_step)
            ids = np.concatenate([ids, ids[: max(1, per_step // 4)], [0, R, R + 7]])   # duplicates, padding, outside
            ls.append(rng.permutation(ids).astype(np.int64))
        g = rng.standard_normal((R, d)).astype(np.float32)
        if tiny_cols:
            g[:, :tiny_cols] *= 1e-8
        out.append((ls, g, 1e-3 * (0.5 + 0.5 * math.cos(t / 17.0)) + 1e-5))
    return (p, m, v), out
