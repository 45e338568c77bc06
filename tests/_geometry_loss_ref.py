"""The geometry loss (losses.fused_geometry_loss) restated for the tests: the formula in the dtype of its
inputs (float64 is the reference of the GPU tests), written from the issue's statement with the explicit-index bilinear
upsample of tests/_masked_loss_ref.py -- not with the package's torch form -- plus the seeded inputs, the shapes and the bounds
every geometry-loss test uses."""
import functools

import numpy as np
import torch

import _masked_loss_ref as MR

# (H, W, th, tw, tanfovx, tanfovy)
CASES = {
    "base": (64, 64, 8, 8, 0.10, 0.10),              # the base case
    "f4x8": (48, 80, 12, 10, 0.15, 0.09),            # factors 4 and 8, tanfovy != tanfovx
    "f1": (40, 24, 40, 24, 0.08, 0.12),              # factor 1: l = 0, the cell unchanged
    "one_cell": (33, 65, 1, 1, 0.12, 0.06),          # one teacher cell; sizes that are no multiple of the 64 x 4 workgroup
    "f2_odd": (130, 70, 65, 35, 0.07, 0.13),         # factor 2 with odd extents
    "workload": (512, 512, 64, 64, 0.149, 0.149),    # the workload's own shape (fov 17 degrees)
}
SMALL = tuple(k for k in CASES if k != "workload")
WEIGHTS = ((0.7, 0.3), (1.0, 0.0), (0.0, 1.0))


def _centres(n):
    return 2 * (torch.arange(n, dtype=torch.float64) + 0.5) / n - 1


def make_inputs(H, W, th, tw, seed=0):
    """float32 (depth [H,W], alpha [H,W], teacher depth [th,tw], teacher weights [th,tw]):
    weights  clip((exp(-3 r^2) - 0.2) / 0.5, 0, 1) * (0.7 + 0.3 U) over the cell centres (an exact-0 rim, never 1);
    teacher depth  2.25 + 1.05 U;
    alpha  a second, wider and off-centre clipped blob * U (exact zeros, never 1, reaching past the weights' support);
    depth  alpha * (2.3 + 0.9 U)."""
    g = torch.Generator().manual_seed(1000 + seed)
    U = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    ty, tx = torch.meshgrid(_centres(th), _centres(tw), indexing="ij")
    w = torch.clip((torch.exp(-3.0 * (tx ** 2 + ty ** 2)) - 0.2) / 0.5, 0.0, 1.0) * (0.7 + 0.3 * U(th, tw))
    t = 2.25 + 1.05 * U(th, tw)
    yy, xx = torch.meshgrid(_centres(H), _centres(W), indexing="ij")
    alpha = torch.clip((torch.exp(-2.0 * ((xx - 0.2) ** 2 + (yy + 0.15) ** 2)) - 0.2) / 0.5, 0.0, 1.0) * U(H, W)
    depth = alpha * (2.3 + 0.9 * U(H, W))
    return depth.float(), alpha.float(), t.float(), w.float()


def maps(t, w, H, W, tanfovx, tanfovy, ray_depth=True):
    """(m, q) [H, W]: the upsampled weights and premultiplied view-space depth, in t's dtype."""
    th, tw = t.shape
    z = t
    if ray_depth:
        xl = (2 * (torch.arange(tw, dtype=t.dtype) + 0.5) / tw - 1) * tanfovx
        yl = (2 * (torch.arange(th, dtype=t.dtype) + 0.5) / th - 1) * tanfovy
        z = t / torch.sqrt(1 + xl[None, :] ** 2 + yl[:, None] ** 2)
    return MR.upsample_mask(w, H, W), MR.upsample_mask(w * z, H, W)


def geometry_loss_ref(depth, alpha, t, w, tanfovx, tanfovy, mask_weight=1.0, depth_weight=1.0, ray_depth=True):
    """(total, terms[3], r_m, r_d, m, q) with 2-D inputs of one dtype."""
    H, W = depth.shape
    m, q = maps(t, w, H, W, tanfovx, tanfovy, ray_depth)
    r_m, r_d = alpha - m, m * depth - alpha * q
    l_m, l_d = r_m.abs().mean(), r_d.abs().mean()
    total = mask_weight * l_m + depth_weight * l_d
    return total, torch.stack([l_m, l_d, total]).detach(), r_m.detach(), r_d.detach(), m, q


def float64_of(depth, alpha, t, w, tanfovx, tanfovy, mask_weight, depth_weight, ray_depth=True):
    """dict of the float64 evaluation on float32 inputs: terms[3], gradients, residuals, m, q and the mask of pixels whose
    sign decision is fragile (0 < |r| <= 1e-5 (|a| + |b|) for r = a - b in either residual)."""
    D, A = depth.double().requires_grad_(True), alpha.double().requires_grad_(True)
    total, terms, r_m, r_d, m, q = geometry_loss_ref(D, A, t.double(), w.double(), tanfovx, tanfovy, mask_weight, depth_weight,
                                                     ray_depth)
    total.backward()
    Dd, Ad = D.detach(), A.detach()
    fragile = ((r_m != 0) & (r_m.abs() <= 1e-5 * (Ad.abs() + m.abs()))) | \
              ((r_d != 0) & (r_d.abs() <= 1e-5 * ((m * Dd).abs() + (Ad * q).abs())))
    return dict(terms=terms.numpy(), grad_depth=D.grad.numpy(), grad_alpha=A.grad.numpy(), r_m=r_m.numpy(), r_d=r_d.numpy(),
                m=m.numpy(), q=q.numpy(), fragile=fragile.numpy())


@functools.lru_cache(maxsize=None)
def case(tag, weights=WEIGHTS[0], ray_depth=True):
    """(float32 inputs, float64 evaluation, float32 torch terms on the CPU) of one case, computed once and shared."""
    H, W, th, tw, tx, ty = CASES[tag]
    inp = make_inputs(H, W, th, tw, seed=sorted(CASES).index(tag))
    ref = float64_of(*inp, tx, ty, weights[0], weights[1], ray_depth)
    terms32 = geometry_loss_ref(*inp, tx, ty, weights[0], weights[1], ray_depth)[1].numpy().astype(np.float64)
    return inp, ref, terms32


def term_bounds(ref_terms, terms32):
    """Per term: the larger of the project's bar for loss terms (tests/test_losses.py: rtol 2e-6 + atol 1e-7) and 4 x the
    deviation of the float32 torch evaluation on the CPU from float64 (the 4: the reduction's other summation order)."""
    return np.maximum(2e-6 * np.abs(ref_terms) + 1e-7, 4.0 * np.abs(terms32 - ref_terms))


def check_gradients(got_depth, got_alpha, ref, mask_weight, depth_weight, scale=1.0):
    """|g - g64| <= 1e-5 |g64| + 1e-6 (mask_weight + depth_weight) / (H W) per pixel outside the fragile pixels, of which a case
    may hold at most 0.1 %.  `scale`: the upstream scalar.  Returns (worst error / bound, pixels left out)."""
    keep = ~ref["fragile"]
    n = keep.size
    left_out = int(n - keep.sum())
    assert left_out <= 1e-3 * n, (left_out, n)
    worst = 0.0
    for got, want in ((got_depth, ref["grad_depth"]), (got_alpha, ref["grad_alpha"])):
        want = scale * want
        err = np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want)
        bound = 1e-5 * np.abs(want) + scale * 1e-6 * (mask_weight + depth_weight) / n
        ratio = (err / bound)[keep]
        worst = max(worst, float(ratio.max()))
    return worst, left_out
