"""float64 restatement of losses.PerceptualStandIn and its two tier twins (the checkers of losses.FusedPerceptual).

`evaluate(module, image, target, max_size, input_affine, tier)` -> dict(loss, grad, features): the stand-in's definition
(lpips.py:16-34 with the stand-in's trunk) in float64, features / loss / image gradient through autograd, with a general
`max_size` (a side above it is averaged down by the integer factor) and `input_affine`.

tier None is the exact restatement.  tier "bf16" / "fp32" is the TWIN of that kernel tier: the same network in float64 with
the kernels' ROUNDING MODEL and nothing else of them --
  * every stored activation (the output of each convolution after its ReLU, i.e. every layer input from conv1_2 on, the pools'
    and the taps' inputs included: max commutes with a monotonic rounding) is rounded to the tier's forward operand format,
    f16 clamped to +-65504 ("bf16") or a split-bf16 pair hi + lo ("fp32");
  * the weights of conv1_2 .. conv5_3 are rounded to that format forward; their backward-data pass uses the weights rounded to
    the backward format, bf16 ("bf16") or the split pair ("fp32");
  * the gradient at every convolution's pre-activation (after the ReLU mask, where the kernels store it) is rounded to the
    backward format;
  * conv1_1, its backward, the taps and all accumulation stay float64 (the kernels: fp32).
"""
import torch
import torch.nn.functional as F

CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
TAPS = (1, 3, 6, 9, 12)


def _f16(x):
    return x.clamp(-65504.0, 65504.0).to(torch.float32).to(torch.float16).to(torch.float64)


def _bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _split(x):
    v = x.to(torch.float32)
    hi = v.to(torch.bfloat16).to(torch.float32)
    return (hi + (v - hi).to(torch.bfloat16).to(torch.float32)).to(torch.float64)


TIERS = {"bf16": (_f16, _bf16), "fp32": (_split, _split)}     # tier -> (forward format, backward format)


class _RoundForward(torch.autograd.Function):     # rounds the value, passes the gradient
    @staticmethod
    def forward(ctx, x, fn):
        return fn(x)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundBackward(torch.autograd.Function):    # passes the value, rounds the gradient
    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


class _TierConv(torch.autograd.Function):         # forward with one weight image, backward-data with another
    @staticmethod
    def forward(ctx, x, w_fwd, w_bwd, bias):
        ctx.save_for_backward(w_bwd)
        ctx.shape = x.shape
        return F.conv2d(x, w_fwd, bias, padding=1)

    @staticmethod
    def backward(ctx, g):
        (w_bwd,) = ctx.saved_tensors
        return torch.nn.grad.conv2d_input(ctx.shape, w_bwd, g, padding=1), None, None, None


def features(module, img, max_size=256, input_affine=None, tier=None):
    """[B, F] float64 rows in PerceptualStandIn.features' order; differentiable in img (float64)."""
    fwd, bwd = TIERS[tier] if tier is not None else (None, None)
    scale, shift = ((2.0,) * 3, (-1.0,) * 3) if input_affine is None else input_affine
    x = img if img.dim() == 4 else img.unsqueeze(0)
    x = x * torch.tensor(scale, dtype=torch.float64)[None, :, None, None] + torch.tensor(shift, dtype=torch.float64)[None, :, None, None]
    if x.shape[2] > max_size:
        assert x.shape[2] % max_size == 0 and x.shape[3] % max_size == 0
        x = F.avg_pool2d(x, (x.shape[2] // max_size, x.shape[3] // max_size))
    feats, ci = [], 0
    for v in CFG:
        if v == "M":
            x = F.max_pool2d(x, 2)
            continue
        w, b = module.convs[ci].weight.detach().double(), module.convs[ci].bias.detach().double()
        if tier is None:
            x = F.relu(F.conv2d(x, w, b, padding=1))
        else:
            z = F.conv2d(x, w, b, padding=1) if ci == 0 else _TierConv.apply(x, fwd(w), bwd(w), b)
            x = _RoundForward.apply(F.relu(_RoundBackward.apply(z, bwd)), fwd)
        if ci in TAPS:
            k = TAPS.index(ci)
            n = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            lin = module.lin[k].detach().double()
            feats.append((n * (lin / (x.shape[2] * x.shape[3])).sqrt()[None, :, None, None]).flatten(1))
        ci += 1
    return torch.cat(feats, 1)


def evaluate(module, image, target, max_size=256, input_affine=None, tier=None):
    """dict(loss: float, grad: float64 tensor like image, features: float64 [B, F] of the image)."""
    img = image.detach().double().requires_grad_(True)
    with torch.no_grad():
        ft = features(module, target.detach().double(), max_size, input_affine, tier)
    fi = features(module, img, max_size, input_affine, tier)
    loss = (fi - ft).square().sum()
    (grad,) = torch.autograd.grad(loss, img)
    return dict(loss=float(loss.detach()), grad=grad.detach(), features=fi.detach())
