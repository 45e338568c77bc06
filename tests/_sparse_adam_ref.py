"""The sparse Adam step of csrc/ggd_adam.hip restated in numpy (the definition the device tests compare bits against), its
float64 counterpart, and the seeded inputs of the tests.

Per element of a visible row, every operation a separate float32 operation in this order:
    m' = (b1 * m) + ((1 - b1) * g)      v' = (b2 * v) + (((1 - b2) * g) * g)      p' = p + (((-lr) * m') / (sqrt(v') + eps))
Rows that are not visible are copied (their bits, NaN payloads included).  No bias correction, no step counter.
"""
import numpy as np

B1, B2 = 0.9, 0.999
EPS = 1e-15
LRS = (0.0, 1.6e-4, 2.5e-3, 0.05)
VISIBILITY = ("all", "none", "every_other", "last", "random30")


def adam32(p, g, m, v, vis, lr, eps=EPS, b1=B1, b2=B2):
    """p, g, m, v: float32 [N, ...]; vis: bool [N].  Returns new (p, m, v), float32."""
    f = np.float32
    assert all(a.dtype == np.float32 for a in (p, g, m, v)) and vis.dtype == np.bool_
    b1, b2, lr, eps, one = f(b1), f(b2), f(lr), f(eps), f(1)
    with np.errstate(all="ignore"):                      # the tests put NaN / Inf into rows that are not visible
        c1 = one - b1
        c2 = one - b2
        t1 = b1 * m
        t2 = c1 * g
        m1 = t1 + t2
        t3 = b2 * v
        t4 = c2 * g
        t5 = t4 * g
        v1 = t3 + t5
        num = (-lr) * m1
        den = np.sqrt(v1) + eps
        q = num / den
        p1 = p + q
    for a in (m1, v1, p1):
        assert a.dtype == np.float32
    out = [p.copy(), m.copy(), v.copy()]
    for o, new in zip(out, (p1, m1, v1)):
        o[vis] = new[vis]
    return tuple(out)


def adam64(p, g, m, v, vis, lr, eps=EPS, b1=B1, b2=B2):
    """The same rule in float64 on the same float32 inputs and float32-rounded constants.  Returns (p, m, v) and the terms the
    rounding bound of the float32 form is built from: |b1 m| + |(1 - b1) g| and sqrt(v') + eps."""
    d = np.float64
    b1, b2, lr, eps = d(np.float32(b1)), d(np.float32(b2)), d(np.float32(lr)), d(np.float32(eps))
    p, g, m, v = (a.astype(d) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = b1 * m + (1.0 - b1) * g
        v1 = b2 * v + (1.0 - b2) * g * g
        den = np.sqrt(v1) + eps
        p1 = p - lr * m1 / den
        mag = np.abs(b1 * m) + np.abs((1.0 - b1) * g)
    rows = vis.reshape((-1,) + (1,) * (p.ndim - 1))
    return (np.where(rows, p1, p), np.where(rows, m1, m), np.where(rows, v1, v)), (mag, den)


def draw_grad(rng, shape, zeros=0.1):
    """|g| log-uniform in [1e-6, 1e2], random sign, a tenth exact zeros: every intermediate of the rule is normal or zero."""
    g = np.exp(rng.uniform(np.log(1e-6), np.log(1e2), size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    g[rng.random(size=shape) < zeros] = 0.0
    return g.astype(np.float32)


def draw_group(rng, N, shape, lr):
    """One group's (p, g, m, v): the moments of two thirds of the rows come from a previous restated step, the rest are zero."""
    shape = (N,) + tuple(shape)
    p = rng.standard_normal(size=shape).astype(np.float32)
    zero = np.zeros(shape, np.float32)
    _, m, v = adam32(p, draw_grad(rng, shape), zero, zero, np.ones(N, bool), lr)
    fresh = rng.random(N) < 1.0 / 3.0
    m[fresh] = 0.0
    v[fresh] = 0.0
    return p, draw_grad(rng, shape), m, v


def visibility(kind, N, rng):
    if kind == "all":
        return np.ones(N, bool)
    if kind == "none":
        return np.zeros(N, bool)
    if kind == "every_other":
        return np.arange(N) % 2 == 0
    if kind == "last":
        return np.arange(N) == N - 1
    if kind == "random30":
        return rng.random(N) < 0.3
    raise ValueError(kind)


def as_radii(vis, rng):
    """int32 radii with the same visible rows: positive there, zero or negative elsewhere."""
    r = np.where(vis, rng.integers(1, 90, size=vis.shape), rng.integers(-3, 1, size=vis.shape)).astype(np.int32)
    assert ((r > 0) == vis).all()
    return r


def widths(M):
    """floats per row of the six groups of a GaussianModel with M SH coefficients per channel"""
    return (3, 3, 3 * (M - 1), 1, 3, 4)
