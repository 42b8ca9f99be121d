"""Reference for the fused SGD with momentum (rs_sgd_step, FusedSGD): torch.optim.SGD(params, lr, momentum=,
weight_decay=) with dampening 0 and nesterov False, the reference trainer's other optimizer.

Per element and step (csrc/sgd_math.h, restated here):
    gj = g            if gs == 1 else g * gs        gs = 1 / the data-parallel count
    gj = fma(wd, p, gj)                 if wd != 0  grad.add(param, alpha=weight_decay)
    b  = (b * momentum) + gj            if momentum buf.mul_(momentum).add_(grad): TWO roundings, no fma
    p  = fma(-lr, b or gj, p)                       param.add_(buf, alpha=-lr)
A zero-initialised buffer gives torch's first-step rule (buf = grad.clone()) from the same line; only the sign of a
zero buffer element can differ (0 * momentum + (-0) = +0), which never reaches p -- buffers are compared by value.

`update` runs it in float64 (the reference: no rounding at all with `scalars(cast=False)`, the kernel's float-cast
hyperparameters with cast=True) or as an emulation of the kernel's float32: every operation rounded to float32, a
fused multiply-add rounded once (the product of two float32 is exact in float64, so one float64 addition and one
rounding to float32 is the fma up to a double rounding in rare ties of the float64 sum -- never seen against torch in
2M element-steps, and inside SLACK of the bound below).

With gs == 1 the emulation equals torch's CPU float32 SGD bit for bit (tests/test_sgd_ref.py), so it is the
yardstick the GPU tests compare the kernel with, bitwise.

The bound of the emulation against float64 (`Bound`; used where gs != 1, where torch offers no float32 yardstick
because it has no gradient scale).  u = 2^-24 is float32's unit roundoff; every float32 operation returns
x (1 + delta), |delta| <= u.  Writing eP, eB for the absolute error bounds of p and b before the step, per element:
    (1) gj0 = fl(g * gs)              e0 = u |g gs|                               (g and gs are exact inputs)
    (2) gj  = fl(wd p + gj0)          eg = e0 + wd eP + u |gj|                    (one rounding: an fma)
    (3) t   = fl(b momentum)          et = momentum eB + u |b momentum|
        b'  = fl(t + gj)              eB' = et + eg + u |b'|                      (the recursion in momentum:
                                          eB' = momentum eB + [u |b momentum| + eg + u |b'|])
    (4) p'  = fl(p - lr x)            eP' = eP + lr ex + u |p'|,  x = b' (ex = eB') or gj (ex = eg)
The four roundings are (1), (2), the two of (3) counted as one line, and (4).  Magnitudes are taken from the float64
run; the difference to the float32 magnitudes is second order (u^2), covered with the fma's double rounding by
SLACK = 1.01 on every step's increment.

MISTAKES names the planted errors tests/test_sgd_ref.py proves these checks reject.
"""
import numpy as np

F32 = np.float32
U32 = 2.0 ** -24
SLACK = 1.01

MISTAKES = ("buf_fma", "decay_after", "lr_in_buf", "first_dampened", "no_clear", "stale_bf16")


def bf16_round(x):
    """float32 array -> the float32 value of its bf16 rounding (round to nearest even; finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def scalars(lr, momentum=0.0, weight_decay=0.0, divisor=None, cast=True):
    """sgd_elem: the hyperparameters cast to float where they meet the tensors (cast=False: the doubles themselves,
    for the comparison with torch on float64 tensors); gs = 1.f / divisor in float32."""
    c = (lambda x: float(F32(x))) if cast else float
    gs = float(F32(1.0) / F32(divisor)) if divisor is not None else 1.0
    return dict(lr=c(lr), mom=c(momentum), wd=c(weight_decay), gs=gs)


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def update(P, G, B, s, dtype=np.float64, first=False, mistake=None):
    """One sgd_elem_update on arrays.  B None: the momentum-free form.  Returns (P, B).  first: the step is the first
    of the run (only the first_dampened mistake reads it)."""
    f32 = dtype == np.float32
    k = {n: dtype(x) for n, x in s.items()}
    P, G = np.asarray(P, dtype=dtype), np.asarray(G, dtype=dtype)
    fma = _fma32 if f32 else (lambda a, b, c: a * b + c)
    gj = G if s["gs"] == 1.0 else G * k["gs"]
    decay = s["wd"] != 0.0
    if decay and mistake != "decay_after":
        gj = fma(k["wd"], P, gj)
    if B is not None:
        B = np.asarray(B, dtype=dtype)
        if mistake == "lr_in_buf":
            gj = gj * k["lr"]
        if mistake == "first_dampened" and first:
            B = (dtype(1.0) - k["mom"]) * gj
        elif mistake == "buf_fma":
            B = fma(B, k["mom"], gj)
        else:
            B = (B * k["mom"]) + gj
        x = B
        if decay and mistake == "decay_after":
            x = fma(k["wd"], P, x)
        P = (P - x) if mistake == "lr_in_buf" else fma(-k["lr"], x, P)
    else:
        P = fma(-k["lr"], gj, P)
    return P, B


class Run:
    """A parameter vector under the rule: p, the accumulated gradient g (backward ADDS into it; the step clears it
    when zero_grad), the momentum buffer (None without momentum) and the bf16 copy of p (as its float32 value)."""

    def __init__(self, p, momentum_on, dtype=np.float64):
        self.dtype = dtype
        self.p = np.array(p, dtype=dtype)
        self.g = np.zeros_like(self.p)
        self.buf = np.zeros_like(self.p) if momentum_on else None
        self.bf16 = bf16_round(np.asarray(p, dtype=np.float32))
        self.t = 0

    def step(self, grad, s, zero_grad=True, mistake=None):
        self.g = self.g + np.asarray(grad, dtype=self.dtype)
        self.p, self.buf = update(self.p, self.g, self.buf, s, self.dtype, first=self.t == 0, mistake=mistake)
        self.t += 1
        if mistake != "stale_bf16":
            self.bf16 = bf16_round(self.p.astype(np.float32))
        if zero_grad and mistake != "no_clear":
            self.g = np.zeros_like(self.g)


class Bound:
    """eP / eB of the module docstring, advanced beside a float64 Run (call before its step, with its state)."""

    def __init__(self, n, momentum_on):
        self.eP = np.zeros(n)
        self.eB = np.zeros(n) if momentum_on else None

    def step(self, ref, grad, s):
        """ref: the float64 Run BEFORE its step(grad, s) (gradient cleared: g = grad)."""
        lr, mom, wd, gs = s["lr"], s["mom"], s["wd"], s["gs"]
        g = np.asarray(grad, np.float64)
        gj = g * gs
        e = U32 * np.abs(gj) if gs != 1.0 else np.zeros_like(gj)
        if wd != 0.0:
            gj = wd * ref.p + gj
            e = e + wd * self.eP + U32 * np.abs(gj)
        if self.eB is not None:
            b1 = ref.buf * mom + gj
            inc = U32 * np.abs(ref.buf * mom) + e + U32 * np.abs(b1)
            self.eB = mom * self.eB + SLACK * inc
            x, ex = b1, self.eB
        else:
            x, ex = gj, SLACK * e
        p1 = ref.p - lr * x
        self.eP = self.eP + lr * ex + SLACK * U32 * np.abs(p1)


# ------------------------------------------------------------------ the checks
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def mismatches(a, b):
    """elements that differ as VALUES (== on every element: +0 equals -0, the one licence a zero-initialised buffer
    needs); NaN never equals"""
    return int(np.count_nonzero(~(np.asarray(a) == np.asarray(b))))


def check_run(run, p, buf=None):
    """Problems (strings; empty = pass) of a float32 Run against another implementation's parameters and buffer:
    == on every element, the bf16 copy the exact rounding of the run's own p, the gradient cleared."""
    bad = []
    if mismatches(run.p, p):
        bad.append(f"p differs in {mismatches(run.p, p)} elements")
    if buf is not None and mismatches(run.buf, buf):
        bad.append(f"buf differs in {mismatches(run.buf, buf)} elements")
    if not same_bits(run.bf16, bf16_round(np.asarray(run.p, np.float32))):
        bad.append("bf16 copy is not the rounding of p")
    if np.count_nonzero(run.g):
        bad.append("gradient not cleared")
    return bad


def scenario(seed, n, steps):
    """Deterministic data: p0 and one gradient per step (a tenth of the entries exactly zero, as the rows of a table
    a batch did not touch)."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    gs = []
    for _ in range(steps):
        g = rng.standard_normal(n).astype(np.float32)
        g[rng.random(n) < 0.1] = 0.0
        gs.append(g)
    return p, gs
