"""TEST-ONLY table of unmasked image-loss cases at the tile, window and block edges of csrc/ggd_imgloss.hip, their float64
yardstick and the per-term bounds of tests/test_image_loss_edges_gpu.py (proved sound from the reference alone by
tests/test_image_loss_cases_host.py).  CPU only; never imported by the product.

Yardstick: _masked_loss_ref.masked_image_loss_torch in float64 (it follows the input dtype and uses the float32-rounded
window, as the kernel does).  `dev32` is the deviation of the SAME restatement run in float32 on this CPU from the float64
one: the size of float32 arithmetic itself on the case, which no float32 kernel can be asked to beat.

Bounds (EPS = 2^-24, half an ulp of 1.0):
  terms L1, L2, Sobel   2e-6 |t64| + 1e-7                                   (the bar of tests/test_losses.py)
  term 1 - SSIM         max(2e-6 |t64| + 1e-7, 4 dev32, 8 EPS)              a difference from 1, so its rounding is in ulps of
                        1.0: S = A1 A2 (1 / (B1 B2)) is five roundings from exact moments, the mean at least one, 1 - . one
                        (on an all-zero pair the reference's x / x is exactly 1, the kernel's reciprocal-then-multiply need
                        not be); the factor 4 as in tests/test_masked_loss_gpu.py (tile partials through float atomics
                        against torch's tree)
  gradient, per element 1e-5 max|g64| for L1, L2, Sobel and the training weights; max(1e-5 max|g64|, 4 dev32_grad) for
                        1 - SSIM (the host test caps 4 dev32_grad at 1e-5 max|g64| for the former and the 1 - SSIM bound at
                        5e-5 max|g64|, so no bound can grow until it hides a failure)
  `equal` (img == tgt)  L1, L2, Sobel: terms and every gradient element exactly 0.  1 - SSIM: the term by its rule; the
                        gradient is a full cancellation (float64 leaves 1e-17 of it, so a bound relative to max|g64| would
                        be a bound of 0): |g| <= max(4 dev32_grad, 16 EPS w max_p piece(p)) with
                        piece = 1/(3HW) (G*|a| + 2|x| G*|b| + |y| G*|c|) from the a, b, c maps of ggd_imgloss.hip's header
                        comment -- sixteen roundings on the pieces that are added.  The training weights on `equal` take
                        this rule too with w = their SSIM weight: the other three gradients are exactly 0 there.
  total                 terms[4] within 4 EPS sum|w_k t_k| of sum w_k terms[k] formed in float64 from the returned float32
                        terms and the float32-rounded weights the kernel is handed (four products, three sums).
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _masked_loss_ref as MR
import _torch_losses as TL

EPS = 2.0 ** -24
SHAPES = ((1, 1), (1, 7), (7, 1), (4, 5), (10, 11), (11, 10), (31, 32), (32, 33), (33, 31), (3, 65), (65, 3), (64, 63), (70, 97))
VARIANTS = ("tex", "black", "over", "equal")
WEIGHTS = collections.OrderedDict(l1=(1.0, 0.0, 0.0, 0.0), l2=(0.0, 1.0, 0.0, 0.0), ssim=(0.0, 0.0, 1.0, 0.0),
                                  sobel=(0.0, 0.0, 0.0, 1.0), train=(0.2, 0.1, 0.5, 0.2))
TERM_NAMES = ("L1", "L2", "1-SSIM", "Sobel")

# t64 / dev_terms: the four terms and the total; g64 [3,H,W]; dev_grad: the largest element of |g32 - g64|
Ref = collections.namedtuple("Ref", "t64 g64 dev_terms dev_grad")


@functools.lru_cache(maxsize=None)
def case(H, W, variant):
    """(image, target) float32 [3,H,W]; the generator is seeded from (H, W) alone."""
    g = torch.Generator().manual_seed(1009 * H + W)
    tgt = torch.rand(3, H, W, generator=g)
    img = tgt + 0.15 * torch.randn(3, H, W, generator=g)                  # not clamped
    img = torch.where(torch.rand(3, H, W, generator=g) < 0.3, tgt, img)   # ~30 % ties
    if variant == "black":
        img, tgt = img.clone(), tgt.clone()
        img[:, :, W // 2:] = 0.0
        tgt[:, :, W // 2:] = 0.0
    elif variant == "over":
        img, tgt = img * 1.6 - 0.3, tgt * 1.6 - 0.3
    elif variant == "equal":
        img = tgt.clone()
    else:
        assert variant == "tex", variant
    return img, tgt


def evaluate(img32, tgt32, weights, mask32=None):
    """Ref of the restatement at the given float32 values: float64, and float32's deviation from it."""
    runs = []
    for dtype in (torch.float64, torch.float32):
        x = img32.detach().to(dtype).requires_grad_(True)
        m = None if mask32 is None else mask32.detach().to(dtype)
        total, terms = MR.masked_image_loss_torch(x, tgt32.detach().to(dtype), *weights, mask=m)
        total.backward()
        runs.append((np.append(terms.detach().numpy().astype(np.float64), float(total.detach())), x.grad.numpy().astype(np.float64)))
    (t64, g64), (t32, g32) = runs
    return Ref(t64, g64, np.abs(t32 - t64), float(np.abs(g32 - g64).max()))


@functools.lru_cache(maxsize=None)
def _ref(H, W, variant, wname):
    return evaluate(*case(H, W, variant), WEIGHTS[wname])


def reference(key, wname):
    """(terms[5], gradient) of the float64 restatement for key = (H, W, variant); cached, not to be written to."""
    r = _ref(*key, wname)
    return r.t64, r.g64


def dev32(key, wname):
    """(|terms32 - terms64|[5], max|g32 - g64|); cached."""
    r = _ref(*key, wname)
    return r.dev_terms, r.dev_grad


def _blur(v):
    """G * v: the 11 x 11 window (float32-rounded taps) with zero padding, per channel, in v's dtype."""
    return F.conv2d(v, TL.create_window(11, 3).to(v.dtype), padding=5, groups=3)


def ssim_pieces(img, tgt):
    """The header comment of ggd_imgloss.hip in float64: (d(1 - SSIM)/d(image), piece), both [3,H,W] numpy, for weight 1."""
    x, y = img.double(), tgt.double()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m1, m2 = _blur(x), _blur(y)
    s11, s22, s12 = _blur(x * x) - m1 * m1, _blur(y * y) - m2 * m2, _blur(x * y) - m1 * m2
    A1, A2, B1, B2 = 2 * m1 * m2 + C1, 2 * s12 + C2, m1 * m1 + m2 * m2 + C1, s11 + s22 + C2
    S = A1 * A2 / (B1 * B2)
    c = 2 * A1 / (B1 * B2)
    b = -S / B2
    a = 2 * m2 * A2 / (B1 * B2) - 2 * m1 * S / B1 - 2 * m1 * b - m2 * c
    n3 = float(x.numel())
    grad = -(_blur(a) + 2 * x * _blur(b) + y * _blur(c)) / n3
    piece = (_blur(a.abs()) + 2 * x.abs() * _blur(b.abs()) + y.abs() * _blur(c.abs())) / n3
    return grad.numpy(), piece.numpy()


@functools.lru_cache(maxsize=None)
def equal_piece_max(H, W):
    return float(ssim_pieces(*case(H, W, "equal"))[1].max())


def term_bounds(ref, exact_zero=False):
    """Bounds of the four terms; exact_zero (the `equal` variant): L1, L2 and Sobel must be exactly 0."""
    tb = 2e-6 * np.abs(ref.t64[:4]) + 1e-7
    tb[2] = max(tb[2], 4.0 * ref.dev_terms[2], 8.0 * EPS)
    if exact_zero:
        tb[[0, 1, 3]] = 0.0
    return tb


def grad_bound(ref, wname, piece_max=None):
    """Per-element gradient bound for upstream factor 1; piece_max: equal_piece_max of an `equal` case."""
    w_ssim = WEIGHTS[wname][2]
    if piece_max is not None:
        return max(4.0 * ref.dev_grad, 16.0 * EPS * w_ssim * piece_max) if w_ssim else 0.0
    bar = 1e-5 * float(np.abs(ref.g64).max())
    return max(bar, 4.0 * ref.dev_grad) if wname == "ssim" else bar


def judge(ref, wname, terms, grad, factor=1.0, piece_max=None, what=""):
    """Asserts the float32 `terms` [5] and `grad` [3,H,W] (with `factor` the upstream gradient) of one kernel call against
    `ref` by the rules of the module docstring; returns the error / bound ratios {term name: r, "grad": r, "total": r}
    (0 / 0 counts as 0)."""
    terms = np.asarray(terms, dtype=np.float64)
    grad = np.asarray(grad, dtype=np.float64)
    assert terms.shape == (5,) and grad.shape == ref.g64.shape, (what, terms.shape, grad.shape)
    assert np.isfinite(terms).all() and np.isfinite(grad).all(), (what, "not every element was written with a finite value")
    tb = term_bounds(ref, exact_zero=piece_max is not None)
    terr = np.abs(terms[:4] - ref.t64[:4])
    assert (terr <= tb).all(), (what, wname, "terms", terms[:4], ref.t64[:4], terr, tb)
    gb = abs(factor) * grad_bound(ref, wname, piece_max)
    gerr = float(np.abs(grad - factor * ref.g64).max()) if piece_max is None else float(np.abs(grad).max())
    assert gerr <= gb, (what, wname, "gradient", gerr, gb)
    w32 = np.asarray(WEIGHTS[wname], dtype=np.float32).astype(np.float64)
    tot_err = abs(terms[4] - float((w32 * terms[:4]).sum()))
    tot_b = 4.0 * EPS * float(np.abs(w32 * terms[:4]).sum())
    assert tot_err <= tot_b, (what, wname, "total", terms, tot_err, tot_b)
    ratio = lambda e, b: 0.0 if e == 0.0 else e / b
    out = {n: ratio(terr[k], tb[k]) for k, n in enumerate(TERM_NAMES)}
    out["grad"], out["total"] = ratio(gerr, gb), ratio(tot_err, tot_b)
    return out


def dev_ratios(ref, wname, piece_max=None):
    """The float32 restatement's own deviation / bound per term and for the gradient: how much of each bound float32
    arithmetic uses up on this CPU."""
    tb = term_bounds(ref, exact_zero=piece_max is not None)
    gb = grad_bound(ref, wname, piece_max)
    ratio = lambda e, b: 0.0 if e == 0.0 else (e / b if b > 0.0 else float("inf"))
    out = {n: ratio(ref.dev_terms[k], tb[k]) for k, n in enumerate(TERM_NAMES)}
    out["grad"] = ratio(ref.dev_grad, gb)
    return out


def keys():
    return [(H, W, v) for (H, W) in SHAPES for v in VARIANTS]
