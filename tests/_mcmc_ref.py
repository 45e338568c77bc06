"""CPU restatement of the MCMC density control (tests/test_mcmc_host.py, tests/test_mcmc_gpu.py): float64 and Python integers.

relocation64()      the relocation values on activated inputs, the double sum as published
raw_values64()      the model-side form: raw opacity / raw scales in, clamped raw opacity / raw scales out, with the condition
                    number sum|terms| / |sum terms| of the alternating sum
raw_values32()      the same expression order in numpy float32 -- the yardstick the bars' constant comes from, never the device
weights_ref() / sample_sources()   the integer sampling plan in Python integers
noise64() / noise_torch32()        the position noise in float64 and as upstream's fp32 torch sequence

Bars (derived here, recorded in DESIGN.md section 6zg):
  value bar    |raw - raw64| <= ATOL + C_REL * 2^-24 * cond.  C_REL = 2 * the largest (err32 - ATOL) / (2^-24 cond) of
               raw_values32 against raw_values64 over value_inputs() (measure_c(): 0 for the opacity, whose fp32 error stays
               under ATOL, and 0.4634 for the scales, at a condition number of up to 8883 at N = 51; C_REL = 0.9268; the
               doubling is for the device's exp / log against libm's).
  noise bar    per row max|dxyz - dxyz64| <= NOISE_RTOL * max|dxyz64|.  NOISE_RTOL = 2 * the largest such ratio of
               noise_torch32 over noise_inputs() (measure_noise_rtol(): 2.976e-4 -- the covariance of scales three decades apart is formed and
               applied in fp32 -- so NOISE_RTOL = 5.95e-4).
"""
from __future__ import annotations

import math

import numpy as np
import torch

N_MAX = 51
O_MIN, O_MAX = 0.005, 1.0 - 2.0 ** -23
WEIGHT_ONE = 1 << 20
ATOL = 1e-5
EPS32 = 2.0 ** -24
C_REL = 0.9268
NOISE_RTOL = 5.95e-4


def relocation64(o, N):
    """o float64 [n] in (0, 1], N int [n] in 1..51 -> (o', o / D, sum|terms| / |D|) with the published double sum."""
    o = np.asarray(o, np.float64)
    N = np.asarray(N, np.int64)
    op = -np.expm1(np.log1p(-o) / N)
    return (op,) + _coefficient64(o, op, N)


def _coefficient64(o, op, N):
    D, A = np.zeros_like(o), np.zeros_like(o)
    for i in range(1, N_MAX + 1):
        live = (N >= i).astype(np.float64)
        for k in range(i):
            term = math.comb(i - 1, k) * ((-1.0) ** k) / math.sqrt(k + 1) * op ** (k + 1) * live
            D += term
            A += np.abs(term)
    return o / D, A / np.abs(D)


def raw_values64(x, raw_scales, N):
    """x float32 [n] raw opacities, raw_scales float32 [n, 3], N int [n] -> (new raw opacity [n], new raw scales [n, 3], cond [n]),
    all float64: o = sigmoid(x), o' = 1 - (1 - o)^(1/N) clamped to [0.005, 1 - 2^-23], logit(o'), log(s o / D)."""
    x = np.asarray(x, np.float64)
    N = np.asarray(N, np.int64)
    sp = np.logaddexp(0.0, x)                             # -log(1 - o)
    t = sp / N
    o, op = -np.expm1(-sp), -np.expm1(-t)
    raw = np.log(np.expm1(t))                             # logit(o')
    raw = np.where(op < O_MIN, math.log(O_MIN / (1 - O_MIN)), np.where(op > O_MAX, math.log(2.0 ** 23 - 1), raw))
    coeff, cond = _coefficient64(o, op, N)
    return raw, np.asarray(raw_scales, np.float64) + np.log(coeff)[:, None], cond


def raw_values32(x, raw_scales, N):
    """The expression order of csrc/ggd_mcmc.hip in numpy float32: softplus, the two expm1, the alternating sum with C(N, k + 1)
    (the inner sums of the published form collapsed) over a running power, log."""
    f = np.float32
    x = np.asarray(x, f)
    Nf = np.asarray(N, np.int64)
    sp = np.where(x > 0, x + np.log1p(np.exp(-x)), np.log1p(np.exp(x))).astype(f)
    t = (sp / Nf.astype(f)).astype(f)
    o, op = (-np.expm1(-sp)).astype(f), (-np.expm1(-t)).astype(f)
    raw = np.log(np.expm1(t).astype(f)).astype(f)
    raw = np.minimum(np.maximum(raw, f(math.log(O_MIN / (1 - O_MIN)))), f(math.log(2.0 ** 23 - 1)))
    D, p = np.zeros_like(op), op.copy()
    for k in range(N_MAX):
        binom = np.array([math.comb(int(n), k + 1) for n in Nf], np.float64).astype(f)
        term = ((binom * p).astype(f) / np.sqrt(f(k + 1))).astype(f)
        D = (D + (term if k % 2 == 0 else -term)).astype(f)
        p = (p * op).astype(f)
    lf = np.log((o / D).astype(f)).astype(f)
    return raw, (np.asarray(raw_scales, f) + lf[:, None]).astype(f)


def value_inputs(seed=0):
    """(x float32 [n], raw scales float32 [n, 3], N int64 [n]): opacities from 0.005 to 1 - 1e-6 (the ends and a log-spaced
    ladder at both of them) against every N in 1..51."""
    ladder = np.concatenate([[0.005, 0.0051, 0.007, 0.01, 0.03, 0.1, 0.3, 0.5, 0.7, 0.9, 0.97],
                             1.0 - np.logspace(-2, -6, 9)])
    o = np.repeat(ladder, N_MAX)
    N = np.tile(np.arange(1, N_MAX + 1), ladder.size)
    x = np.log(o / (1 - o)).astype(np.float32)
    gen = np.random.default_rng(seed)
    return x, gen.uniform(-7.0, 1.0, (x.size, 3)).astype(np.float32), N.astype(np.int64)


def measure_c():
    """The constant of the value bar before doubling, (opacity, scales)."""
    x, s, N = value_inputs()
    raw64, s64, cond = raw_values64(x, s, N)
    raw32, s32 = raw_values32(x, s, N)
    unit = EPS32 * cond
    return (float((np.maximum(np.abs(raw32 - raw64) - ATOL, 0) / unit).max()),
            float((np.maximum(np.abs(s32 - s64) - ATOL, 0) / unit[:, None]).max()))


# ---- the integer sampling plan ------------------------------------------------------------------------------------------
def weights_ref(o, dead):
    """o float64 [n], dead bool [n] -> list of Python ints."""
    return [0 if d else max(1, int(round(float(v) * WEIGHT_ONE))) for v, d in zip(o, dead)]


def sample_sources(weights, draws):
    """weights: ints [n]; draws: {destination: d in [0, 2^32)} or a list (destination k = k-th entry).  Returns (sources in
    the order of the destinations, counts [n]).  tau = floor(d W / 2^32); the source is the row whose half-open interval
    [C_i, C_i + w_i) of the exclusive prefix sum holds tau.  W == 0: no sources."""
    import bisect
    items = sorted(draws.items()) if isinstance(draws, dict) else list(enumerate(draws))
    counts = [0] * len(weights)
    W = sum(weights)
    if W == 0:
        return [-1] * len(items), counts
    ends, run = [], 0
    for w in weights:
        run += w
        ends.append(run)                                  # inclusive prefix: the source is the first row with end > tau
    sources = []
    for _, d in items:
        assert 0 <= d < 1 << 32
        tau = (d * W) >> 32
        s = bisect.bisect_right(ends, tau)
        assert weights[s] > 0 and ends[s] - weights[s] <= tau < ends[s]
        sources.append(s)
        counts[s] += 1
    return sources, counts


# ---- position noise -----------------------------------------------------------------------------------------------------
def _rotation(q):
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


def noise64(raw_scales, rotation, x, xi, noise_lr, xyz_lr):
    """dxyz in float64 from fp32 inputs: Sigma (gate noise_lr xyz_lr xi), gate = sigmoid(100 (sigmoid(-x) - 0.995))."""
    s, q, x, xi = (t.double() for t in (raw_scales, rotation, x.reshape(-1), xi))
    L = _rotation(q) * torch.exp(s)[:, None, :]
    gate = torch.sigmoid(100.0 * (torch.sigmoid(-x) - 0.995))
    return torch.bmm(L @ L.transpose(1, 2), (xi * gate[:, None] * noise_lr * xyz_lr)[..., None]).squeeze(-1)


def noise_torch32(raw_scales, rotation, x, xi, noise_lr, xyz_lr):
    """Upstream's lines in fp32 torch on the CPU: L = R S, covariance = L L^T, noise = randn * op_sigmoid(1 - opacity) *
    noise_lr * xyz_lr, bmm(covariance, noise)."""
    L = _rotation(rotation) @ torch.diag_embed(torch.exp(raw_scales))
    cov = L @ L.transpose(1, 2)
    gate = 1 / (1 + torch.exp(-100 * ((1 - torch.sigmoid(x.reshape(-1, 1))) - 0.995)))
    noise = xi * gate * noise_lr * xyz_lr
    return torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1)


def noise_inputs(P, seed):
    """Raw scales (anisotropic over three decades), raw quaternions, raw opacities from o = 6e-6 to o = 0.62, xi."""
    gen = torch.Generator().manual_seed(seed)
    s = -7.0 + 7.0 * torch.rand((P, 3), generator=gen)
    q = torch.randn((P, 4), generator=gen) + 0.1
    x = -12.0 + 12.5 * torch.rand((P, 1), generator=gen)
    if P >= 8:
        x[:4] = torch.tensor([[-12.0], [-8.0], [0.0], [0.0]])   # gate 0.62, 0.62, and o = 0.5 twice
    return s, q, x, torch.randn((P, 3), generator=gen)


def noise_row_error(got, ref64):
    """per row max|got - ref| / max|ref|"""
    return ((got.double() - ref64).abs().amax(dim=1) / ref64.abs().amax(dim=1).clamp_min(1e-300))


def measure_noise_rtol(sizes=(1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 7, 20_011), noise_lr=5e5, xyz_lr=1.6e-4):
    worst = 0.0
    for P in sizes:
        s, q, x, xi = noise_inputs(P, P)
        worst = max(worst, float(noise_row_error(noise_torch32(s, q, x, xi, noise_lr, xyz_lr),
                                                 noise64(s, q, x, xi, noise_lr, xyz_lr)).max()))
    return worst
