"""Reference for the global gradient norm and clip coefficient (csrc/gradnorm.hip: rs_gradnorm_dense, rs_gradnorm_rows,
rs_gradnorm_finish; FusedTrainStep(max_grad_norm=)).

What is computed, as torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=False) forms it:
    norm = sqrt(sum g^2) / div                          div: the step's gradient divisor, or 1
    coef = min(1, max_norm / (norm + 1e-6))
    eff  = div                          if coef == 1    the divisor the optimizer kernels take (gs = 1 / eff)
           div * (norm + 1e-6) / max_norm   otherwise

`reference` forms the three in extended precision (np.longdouble sums: the reference's own error, n * 2^-64 on x86, is
far below the bounds; where longdouble is a double the pairwise sum's log2(n) * 2^-53 still is).

`emulate_*` restate the kernels' partial order in numpy float64 (IEEE double addition, the same on both sides):
  a range / list is summed by a VIRTUAL grid of nv workgroups of 256 threads, nv from the length alone (dense_parts,
  rows_parts); thread t of workgroup v takes the items (float4s, or single elements on the scalar row path)
  v * 256 + t + k * nv * 256, k = 0, 1, ..., in that order, into one accumulator per float4 component; a dense range's
  n % 4 tail goes to threads t < n % 4 of workgroup 0, component 0; then (s0 + s1) + (s2 + s3), a 64-lane xor butterfly
  (offsets 32 .. 1), ((w0 + w1) + w2) + w3 over the waves: one partial per virtual workgroup, zeros included.  The
  finish: thread t adds the slots t, t + 256, ...; the same block sum; then the scalar lines below.

The bounds.  u = 2^-53 (double), U = 2^-24 (float).  The square of a float is exact in double (48 <= 53 bits), and
adding a zero is exact, so only additions of two non-zero terms round.  Each such addition on the path of one element
to the total merges two non-empty sets of elements, so a path holds at most n - 1 of them, whatever the order (any
grid, any partial layout): computed sum = sum_i g_i^2 (1 + t_i), |t_i| <= (n - 1) u to first order, and since every
term is non-negative the sum's relative error is at most (n - 1) u.  Then, one rounding each:
    sqrt            halves the sum's error: (n - 1) u / 2 + u
    / div           + u              (div is a float: exact as a double)
    (float)         + U
  NORM_REL(n) = U + (n + 4) u                >= U + ((n - 1) / 2 + 2) u: |norm - ref| <= ref (2^-24 + n 2^-53) for
                                             the sum and the cast, 4 u for the sqrt's and the division's roundings
    e = norm + 1e-6 + u   ->  coef = (float)(max_norm / e): + u + U      COEF_REL(n) = U + (n + 6) u
                              eff  = (float)(div * e / max_norm): + 2 u + U       EFF_REL(n) = U + (n + 7) u
As ulp counts (one ulp = 2^-24 |ref|, the half-spacing bound of round-to-nearest): 1 + (n + 4) / 2^29 for the norm,
1 + (n + 6) / 2^29 for the coefficient, 1 + (n + 7) / 2^29 for the divisor -- 1.03 ulps at the 2^24 elements of the
largest test.  Second-order terms ((n u)^2 = 2^-58 there) sit inside the (n / 2 + 2) u the first-order bounds leave.
A coefficient that rounds to 1 on one side of the clamp and to just below it on the other is inside the same bounds:
both branches are continuous there.

MISTAKES names the planted errors tests/test_gradnorm_ref.py proves these checks reject.
"""
import numpy as np

NT, U_ITEMS, DENSE_VB, ROWS_VB = 256, 4, 2048, 1024
U64, U32 = 2.0 ** -53, 2.0 ** -24
EPS = 1e-6

MISTAKES = ("tail_dropped", "cap_not_count", "last_row_dropped", "abs_not_square", "divisor_ignored", "no_clamp",
            "no_eps", "bias_list_omitted", "stale_partials")


def _cdiv(a, b):
    return -(-a // b)


def dense_parts(n):
    return min(max(_cdiv(n // 4, NT * U_ITEMS), 1), DENSE_VB)


def rows_parts(d, cap):
    return min(max(_cdiv(cap * d, 4 * NT * U_ITEMS), 1), ROWS_VB)


def norm_rel(n):
    return U32 + (n + 4) * U64


def coef_rel(n):
    return U32 + (n + 6) * U64


def eff_rel(n):
    return U32 + (n + 7) * U64


# ------------------------------------------------------------------ the reference
def sumsq(*arrays):
    """sum of squares of float32 arrays, in extended precision"""
    tot = np.longdouble(0)
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        tot += np.sum(a * a, dtype=np.longdouble)
    return tot


def reference(ss, max_norm, div=None):
    """(norm, coef, eff) as Python floats from the sum of squares ss"""
    dv = np.longdouble(1.0 if div is None else float(np.float32(div)))
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.longdouble(ss)) / dv
        c = np.longdouble(max_norm) / (norm + np.longdouble(EPS))
        clip = not c >= 1
        eff = dv * (norm + np.longdouble(EPS)) / np.longdouble(max_norm) if clip else dv
    return float(norm), float(c) if clip else 1.0, float(eff)


def check_record(rec, ref, n):
    """Problems (strings; none when it passes) of a float32 record {norm, coef, eff} against `reference`'s triple for
    a norm over n elements."""
    bad = []
    for name, got, want, r in zip(("norm", "coef", "eff"), rec, ref, (norm_rel(n), coef_rel(n), eff_rel(n))):
        got = float(got)
        if not np.isfinite(want):
            if not (got == want or (np.isnan(got) and np.isnan(want))):
                bad.append(f"{name}: {got} against {want}")
        elif not abs(got - want) <= r * abs(want):
            bad.append(f"{name}: {got!r} against {want!r}: off by {abs(got - want) / max(abs(want), 1e-300):.3g} "
                       f"> {r:.3g}")
    return bad


# ------------------------------------------------------------------ the kernels' order
def _block_sum(v):
    """v [nv, 256] float64 -> [nv]: the butterfly over each wave's 64 lanes, then ((w0 + w1) + w2) + w3"""
    v = v.reshape(-1, NT // 64, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _items_partials(items, nv, tail=None, square=True):
    """items float32 [m, 4] (unused components zero) -> the nv partials; tail: up to 3 elements for workgroup 0"""
    x = np.asarray(items, dtype=np.float64).reshape(-1, 4)
    x = x * x if square else np.abs(x)
    stride = nv * NT
    K = max(_cdiv(x.shape[0], stride), 1)
    pad = np.zeros((K * stride, 4))
    pad[:x.shape[0]] = x
    s = np.zeros((nv, NT, 4))
    for blk in pad.reshape(K, nv, NT, 4):
        s = s + blk
    if tail is not None and len(tail):
        t = np.asarray(tail, dtype=np.float64)
        s[0, :len(t), 0] = s[0, :len(t), 0] + (t * t if square else np.abs(t))
    return _block_sum((s[:, :, 0] + s[:, :, 1]) + (s[:, :, 2] + s[:, :, 3]))


def emulate_dense(g, ranges, mistake=None):
    """rs_gradnorm_dense: the partials of every range, back to back"""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    out = []
    for lo, hi in ranges:
        x = g[lo:hi]
        n4 = x.size // 4
        tail = None if mistake == "tail_dropped" else x[4 * n4:]
        out.append(_items_partials(x[:4 * n4], dense_parts(x.size), tail, square=mistake != "abs_not_square"))
    return np.concatenate(out)


def emulate_rows(table, rows, count, cap, ws=None, mistake=None, vec=None):
    """rs_gradnorm_rows on the list rows[:count] (capacity cap) of table [R][d]: all rows_parts(d, cap) partials.  ws:
    the slots' previous content (only the stale_partials mistake keeps any of it)."""
    table = np.asarray(table, dtype=np.float32)
    table = table.reshape(table.shape[0], -1)
    R, d = table.shape
    nv = rows_parts(d, cap)
    n = min(max(int(count), 0), cap)
    if mistake == "cap_not_count":
        n = cap
    if mistake == "last_row_dropped":
        n = max(n - 1, 0)
    ids = np.asarray(rows[:n], dtype=np.int64)
    ok = (ids >= 0) & (ids < R)
    picked = np.zeros((n, d), np.float32)         # an id outside the table keeps its items, as zeros
    picked[ok] = table[ids[ok]]
    vec = d % 4 == 0 if vec is None else vec
    if vec:
        items = picked.reshape(-1, 4)
    else:
        items = np.zeros((picked.size, 4), np.float32)
        items[:, 0] = picked.reshape(-1)
    part = _items_partials(items, nv, square=mistake != "abs_not_square")
    if mistake == "stale_partials" and ws is not None:
        used = _cdiv(items.shape[0], NT)            # workgroups without an item return before their store
        part[used:] = np.asarray(ws)[used:nv]
    return part


def emulate_finish(partials, max_norm, div=None, mistake=None):
    """rs_gradnorm_finish -> float32 [3] = {norm, coef, effective divisor}"""
    p = np.asarray(partials, dtype=np.float64).reshape(-1)
    pad = np.zeros(_cdiv(max(p.size, 1), NT) * NT)
    pad[:p.size] = p
    s = np.zeros(NT)
    for blk in pad.reshape(-1, NT):
        s = s + blk
    tot = float(_block_sum(s.reshape(1, NT))[0])
    dv = np.float32(1.0 if div is None else div)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(np.float64(tot)) / np.float64(1.0 if mistake == "divisor_ignored" else dv)
        e = nrm + (0.0 if mistake == "no_eps" else EPS)
        mx = np.float64(max_norm)
        coef = np.float32(mx / e)
        clip = not coef >= np.float32(1.0)
        if mistake == "no_clamp":
            clip = True
        eff = np.float32(np.float64(dv) * e / mx) if clip else dv
    return np.array([np.float32(nrm), coef if clip else np.float32(1.0), eff], dtype=np.float32)


def emulate_step(g, segs, tables, max_norm, div=None, mistake=None, ws=None):
    """The step's launches: dense partials over segs = [(lo, hi)], row partials over tables = [(lo, rows, d, list,
    count)] of the flat gradient g, the finish.  Returns (record, workspace)."""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    parts = [emulate_dense(g, segs, mistake)] if segs else []
    at = sum(p.size for p in parts)
    for k, (lo, rows, d, lst, cnt) in enumerate(tables):
        if mistake == "bias_list_omitted" and d == 1:
            parts.append(np.zeros(rows_parts(d, len(lst))))
        else:
            old = None if ws is None else ws[at:]
            parts.append(emulate_rows(g[lo:lo + rows * d].reshape(rows, d), lst, cnt, len(lst), old, mistake))
        at += parts[-1].size
    ws = np.concatenate(parts)
    return emulate_finish(ws, max_norm, div, mistake), ws
