"""TEST-ONLY restatement of the fused decoder (csrc/ggd_mlp*.{hip,inc}): a manual forward and backward of
SequentialDecoderReverse's five-head chain on plane features, in plain torch ops, any dtype, CPU or device, with a
rounding hook at every place where the kernels round.  With identity hooks in float64 it IS the module's autograd
(tests/test_decoder_ref_host.py holds it to 1e-12); with a tier's hooks it is the yardstick of that tier's rounding noise:
the GPU tests allow a kernel four times the deviation of its tier's restatement from float64, never a figure taken from
the kernel.  The float64 side always uses the exact GELU / GELU'; the bf16 tier's preset carries that tier's polynomials as
rounding points (see BF16_TIER), each held to its documented error on the CPU.
Never imported by the product.

The chain, as the kernels compute it (head order colour, opacity, rotation, scale, xyz; attrs[N,16] columns 0..2, 3, 4..7,
8..10, 11..13):
  forward, head h:   x0 = [feat(32) | pos(3) | attrs[:, :A0[h]]],  z_l = a_{l-1} W_l^T + b_l,  a_l = gelu(z_l)  (l = 1..3),
                     raw = a_3 W_4^T + b_4;  scale = -softplus(raw + 5) - 2.5,  xyz = 0.01 raw + pos
  backward, h = 4..0: d = dattrs[:, cols(h)]  (+ what the later heads sent back through `info`;  xyz: * 0.01;
                     scale: * -sigmoid(raw + 5), recovered from the activated value as -(1 - exp(-softplus)))
                     dh = d W_4,  dz_l = dh * gelu'(z_l),  dh = dz_l W_l  (l = 3, 2, 1);
                     dfeat += dh[:, :32],  dinfo += dh[:, 32:];   dW_l = dz_l^T a_{l-1},  db_l = sum dz_l  (dz_4 = d)
"""
import math
from types import SimpleNamespace

import torch

A0 = (0, 3, 4, 8, 11)         # first attrs column of a head == number of chained inputs it sees
OD = (3, 1, 4, 3, 3)          # output width
SLAB = 32                     # points that share one power-of-two scale in the reference-precision tier
HEADS = ("color_decoder", "opacity_decoder", "rotation_decoder", "scale_decoder", "xyz_decoder")


def gelu(x):
    return x * (0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


# ---- the bf16 tier's polynomials (coefficients as in the kernel sources; tests/test_decoder_ref_host.py holds each to the error
#      its source documents against the exact function, so a wrong coefficient HERE cannot excuse one in a kernel) -------------
def _f32(fn):
    return lambda x: fn(x.float()).to(x.dtype)


@_f32
def gelu_f16_poly(z):
    """gelu_h2x4 (ggd_mlp.hip), the f16 forward's GELU: y = z / 2, a = |y|, v = min(a, 2) - 1, gelu = y + a s(v), s of degree 6,
    every step rounded to f16 (a packed-f16 fma rounds once; the f16 x f16 product is exact in fp32)"""
    h = lambda t: t.half().float()
    S = (9.546607429e-01, 2.169445321e-01, -4.391409802e-01, 4.247604060e-01, -9.772952171e-02, -1.414002710e-01, 8.190509189e-02)
    y = h(z * 0.5)
    a = y.abs()
    v = h(a.clamp(max=2.0) - 1.0)
    p = h(v * h(torch.tensor(S[6])) + h(torch.tensor(S[5])))
    for k in range(4, -1, -1):
        p = h(p * v + h(torch.tensor(S[k])))
    return h(a * p + y)


def _odd_poly(x, coeffs):
    xc = x.clamp(-4.0, 4.0)
    s2 = xc * xc
    p = torch.full_like(x, coeffs[0])
    for c in coeffs[1:]:
        p = p * s2 + c
    return xc * p + 0.5


@_f32
def gelu_poly(x):
    """gelu2x4 (ggd_mlp.hip), the weight-gradient kernel's recomputed activation: x (0.5 + xc P7(xc^2)) in fp32"""
    return x * _odd_poly(x, (-1.520480094e-09, 1.180964698e-07, -4.014221549e-06, 7.960997496e-05, -1.041295812e-03,
                             9.641715482e-03, -6.614117560e-02, 3.988329117e-01))


@_f32
def gelu_grad_poly(x):
    """gelu_grad2x4 (ggd_mlp_bwd.inc): 0.5 + xc P7(xc^2) in fp32, max |error| 3.1e-4"""
    return _odd_poly(x, (-1.557768258e-08, 1.163350639e-06, -3.725065996e-05, 6.728997635e-04, -7.591166539e-03,
                         5.559237280e-02, -2.615541427e-01, 7.965189430e-01))


# ---- number formats ---------------------------------------------------------------------------------------------------------
def _via(x, dtype):
    return x.to(dtype).to(x.dtype)


def r_bf16(x):
    return _via(x, torch.bfloat16)


def r_f16(x):
    """fp32 -> f16, saturating at +-65504 as every f16 conversion of the kernels does"""
    return _via(x.clamp(-65504.0, 65504.0), torch.float16)


def split_hl(x):
    """fp32 -> its (hi, lo) bf16 parts (split8 in ggd_mlp_hl.inc, the pack kernel's bf16 hi / lo formats): hi = bf16(x),
    lo = bf16(x - hi), both from the fp32 value"""
    x32 = x.float()
    hi = x32.bfloat16()
    return hi, (x32 - hi.float()).bfloat16()


def r_hl(x):
    """hi + lo bf16 (split_hl), summed"""
    hi, lo = split_hl(x)
    return (hi.double() + lo.double()).to(x.dtype)


class GradIdentity:
    """Fourth hook: how the gradient planes are rounded.  begin_head(d) is told the gradient at the head's raw output before
    anything of that head is rounded; operand(x) rounds d / dz where it becomes the next product's operand in the activation
    backward; wgrad(left, right) rounds the two operands of a weight-gradient product dW = left^T right (left = dz or d,
    right = a_{l-1} with a trailing column of ones for the bias gradient) and returns them at their true scale."""

    def begin_head(self, d):
        pass

    def operand(self, x):
        return x

    def wgrad(self, left, right):
        return left, right


class GradBf16(GradIdentity):
    """decoder_backward_kernel / decoder_wgrad_kernel: dz is ONE bf16 plane, both the next operand and the left operand of the
    weight gradient; dout (layer 4) and the right operand (gelu(z) recomputed in fp32, or the fp32 inputs) are rounded to bf16."""

    def operand(self, x):
        return r_bf16(x)

    def wgrad(self, left, right):
        return r_bf16(left), r_bf16(right)


class GradHl(GradIdentity):
    """decoder_backward_hl_kernel / decoder_wgrad_hl_kernel: dz enters the next product split (hi + lo); it is stored as fp16
    after the power-of-two scale of its (head, 32-point slab): frexp of the slab's largest |d| gives the exponent ke,
    S = 2^(4 - ke) puts it in [8, 16).  The weight gradient multiplies the slab's right operand by 2^(ks - km) (km: the
    largest ke of the head; never below 2^-80), rounds it to fp16, and scales the sums by 2^(km - 4).  A slab without a
    gradient (ke undefined) contributes nothing."""

    def begin_head(self, d):
        n = d.shape[0]
        nslab = (n + SLAB - 1) // SLAB
        dm = torch.zeros(nslab * SLAB, dtype=torch.float32, device=d.device)
        dm[:n] = d.float().abs().amax(1)
        dmax = dm.view(nslab, SLAB).amax(1)
        ke = torch.frexp(dmax)[1].to(torch.int64)
        valid = (dmax > 0) & (dmax <= 3.0e38)
        km = ke[valid].max() if bool(valid.any()) else torch.zeros((), dtype=torch.int64, device=d.device)
        two = torch.full((), 2.0, dtype=torch.float64, device=d.device)
        S = torch.where(valid, torch.pow(two, (4 - ke).double()), torch.ones_like(dmax, dtype=torch.float64))
        fB = torch.where(valid, torch.pow(two, (ke - km).clamp_min(-80).double()), torch.zeros_like(S))
        self.S = S.repeat_interleave(SLAB)[:n, None]
        self.fB = fB.repeat_interleave(SLAB)[:n, None]

    def operand(self, x):
        return r_hl(x)

    def wgrad(self, left, right):
        S, fB = self.S.to(left.dtype), self.fB.to(right.dtype)
        L = r_f16(left * S) / S
        return L, r_f16(right * fB) / fB.clamp_min(2.0 ** -90)      # fB = 0: the rounded product is 0 already


class Tier:
    """The four hooks (+ where the forward's GELU starts from).  fwd: operands of the forward products (inputs, weights,
    activations); z: the pre-activation as it is stored for the backward; wt: the transposed weights of the activation
    backward; grad: a Grad* object (dz / dout and the right operand of the weight-gradient product).
    gelu_of_stored_z: the f16 forward's GELU starts from the SAME f16 conversion that is stored (gelu_pack in ggd_mlp.hip);
    the reference-precision forward applies it to the fp32 accumulator and rounds only the stored copy."""

    def __init__(self, name, fwd, z, wt, grad, gelu_of_stored_z, act=gelu, act_wg=gelu, dact=gelu_grad):
        self.name, self.fwd, self.z, self.wt, self.grad, self.gelu_of_stored_z = name, fwd, z, wt, grad, gelu_of_stored_z
        # the activation of the forward, the one the weight gradient recomputes from the stored z, and its derivative: exact
        # unless the tier's approximation is itself a rounding point of the size of the others (BF16_TIER below)
        self.act, self.act_wg, self.dact = act, act_wg, dact


def _same(x):
    return x


IDENTITY = Tier("float", _same, _same, _same, GradIdentity, False)
# precision="bf16": f16 forward operands and z (ggd_mlp.hip), bf16 transposed weights and dz (ggd_mlp_bwd.inc), bf16 gelu(z) and
# inputs in the weight gradient (ggd_mlp_wgrad.inc)
# Its GELUs are polynomials whose documented errors (forward, in packed f16: 1.5e-3; gelu': 3.1e-4; recomputed gelu: 2e-4) are of
# the size of the roundings next to them (f16: 4.9e-4, bf16: 3.9e-3 relative): with the exact functions here, a float32 evaluation
# of this preset WITH the polynomials -- a stand-in for a correct kernel -- lay 5.8 dev off float64 in the opacity head's output
# bias (one element, a sum of signed terms) at N = 255 and up to 6.2 dev in the attributes, so they are rounding points of the
# tier.  The reference-precision tier's tables (1e-6) are far below its fp16 roundings (2.4e-4) and stay exact.
BF16_TIER = Tier("bf16", r_f16, r_f16, r_bf16, GradBf16, True, act=gelu_f16_poly, act_wg=gelu_poly, dact=gelu_grad_poly)
# precision="fp32": split operands everywhere, z one fp16 plane, dz one scaled fp16 plane (ggd_mlp_hl.inc)
FP32_TIER = Tier("fp32", r_hl, r_f16, r_hl, GradHl, False)
TIERS = {"bf16": BF16_TIER, "fp32": FP32_TIER}


def module_params(mod, dtype=None, device=None):
    """The 40 tensors (W1 b1 .. W4 b4 per head, head order) == the order of SequentialDecoderReverse.named_parameters()"""
    out = []
    for name in HEADS:
        bb = getattr(mod, name).backbone
        for k in (0, 2, 4, 6):
            out += [bb[k].weight.detach(), bb[k].bias.detach()]
    return [p.to(dtype=dtype or p.dtype, device=device or p.device) for p in out]


def decoder_ref(params, feats, pos, dattrs, tier=IDENTITY):
    """params: 40 tensors (module_params), feats [N,32], pos [N,3], dattrs [N,16] (columns 14, 15 ignored), all of one dtype and
    device -> attrs [N,16], dfeat [N,32], dinfo [N,16] (slots 0..2 position, 3 + k attrs column k), dout [5,N,4], grads (40)."""
    n = pos.shape[0]
    kw = dict(dtype=feats.dtype, device=feats.device)
    attrs = torch.zeros((n, 16), **kw)
    zs, x0s = [], []
    for h in range(5):
        W = params[8 * h:8 * h + 8]
        x0 = torch.cat([feats, pos, attrs[:, :A0[h]]], 1)
        a, zh = x0, []
        for l in range(3):
            z = tier.fwd(a) @ tier.fwd(W[2 * l]).t() + W[2 * l + 1]
            zh.append(tier.z(z))
            a = tier.act(zh[-1] if tier.gelu_of_stored_z else z)
        raw = tier.fwd(a) @ tier.fwd(W[6]).t() + W[7]
        if h == 3:
            raw = -torch.nn.functional.softplus(raw + 5.0) - 2.5
        elif h == 4:
            raw = raw * 0.01 + pos
        attrs[:, A0[h]:A0[h] + OD[h]] = raw
        zs.append(zh)
        x0s.append(x0)

    dfeat = torch.zeros((n, 32), **kw)
    dinfo = torch.zeros((n, 16), **kw)
    dout = torch.zeros((5, n, 4), **kw)
    grads = [None] * 40
    ones = torch.ones((n, 1), **kw)
    for h in range(4, -1, -1):
        W = params[8 * h:8 * h + 8]
        grad = tier.grad()
        d = dattrs[:, A0[h]:A0[h] + OD[h]].clone()
        if h == 4:
            d = d * 0.01
        else:
            d = d + dinfo[:, 3 + A0[h]:3 + A0[h] + OD[h]]
            if h == 3:
                sp = -attrs[:, 8:11] - 2.5
                d = d * -(1.0 - torch.exp(-sp))
        dout[h, :, :OD[h]] = d
        grad.begin_head(d)

        def wg(left, right, slot):
            L, R = grad.wgrad(left, torch.cat([right, ones], 1))
            g = L.t() @ R
            grads[8 * h + 2 * slot], grads[8 * h + 2 * slot + 1] = g[:, :-1], g[:, -1]

        wg(d, tier.act_wg(zs[h][2]), 3)
        dh = grad.operand(d) @ tier.wt(W[6])
        for l in (2, 1, 0):
            dz = dh * tier.dact(zs[h][l])
            wg(dz, tier.act_wg(zs[h][l - 1]) if l else x0s[h], l)
            dh = grad.operand(dz) @ tier.wt(W[2 * l])
        dfeat = dfeat + dh[:, :32]
        dinfo[:, :dh.shape[1] - 32] += dh[:, 32:]
    return SimpleNamespace(attrs=attrs, dfeat=dfeat, dinfo=dinfo, dout=dout, grads=grads)


# ---- the seeded inputs of the tests (host and GPU tests share them) -----------------------------------------------------------
def make_decoder(seed=3):
    """The seeded module with its 2-D parameters * 1.5 (heads' outputs O(1), as tests/test_decoder_gpu.py does)"""
    from gaussian_gan_decoder_amd.decoder import SequentialDecoderReverse
    torch.manual_seed(seed)
    mod = SequentialDecoderReverse()
    for p in mod.parameters():
        if p.dim() == 2:
            p.data *= 1.5
    return mod


def make_inputs(n, seed=0):
    """CPU float32: feats = 0.6 randn [n,32], pos uniform in [-0.5, 0.5) [n,3], dattrs = randn [n,16] with columns 14, 15 zero"""
    g = torch.Generator().manual_seed(1000 + seed)
    feats = 0.6 * torch.randn(n, 32, generator=g)
    pos = torch.rand(n, 3, generator=g) - 0.5
    dattrs = torch.randn(n, 16, generator=g)
    dattrs[:, 14:] = 0
    return feats, pos, dattrs


def zero_point_mask(n):
    """The zero-gradient pattern: points 64..159 (three whole slabs) and every third point elsewhere get dattrs = 0"""
    idx = torch.arange(n)
    return ((idx >= 64) & (idx < 160)) | (idx % 3 == 0)


def colour_only(dattrs):
    d = torch.zeros_like(dattrs)
    d[:, 0:3] = dattrs[:, 0:3]
    return d


# ---- the reference-precision tier's weight images (the 16-bit tier's host statement is fused_decoder.pack_weights / _t) ----------
def pack_hl_host(mod):
    """TEST-ONLY host statement of what ggd_decoder_pack_hl writes: (packed_hl, packed_t_hl) as uint8 tensors.  Rows are
    permuted and swizzled exactly like the 16-bit images (fused_decoder._permute_blocks / _swizzle_rows); every matrix is two
    bf16 images, hi then lo (split_hl).
      forward, per head   : [L1 hi | L1 lo | L2 hi | L2 lo | L3 hi | L3 lo | L4 hi | L4 lo | b1 b2 b3 b4(16) fp32], nothing halved
                            (L1 = W1 [128][64], K padded with zeros; L4 = W4 [16][128], rows padded with zeros)
      transposed, per head: [W4^T hi | lo | W3^T hi | lo | W2^T hi | lo | W1^T hi | lo], W4^T [128][32 + 8] padded and not
                            swizzled, W1^T [64][128]"""
    from gaussian_gan_decoder_amd import fused_decoder as FD
    p = module_params(mod, dtype=torch.float32)
    dev = p[0].device
    as_bytes = lambda t: t.contiguous().view(torch.uint8).reshape(-1)
    fwd, bwd = [], []
    for h in range(5):
        w1, b1, w2, b2, w3, b3, w4, b4 = p[8 * h:8 * h + 8]
        w1f = torch.zeros(128, 64, device=dev); w1f[:, :w1.shape[1]] = w1
        w4f = torch.zeros(16, 128, device=dev); w4f[:w4.shape[0]] = w4
        b4f = torch.zeros(16, device=dev); b4f[:b4.shape[0]] = b4
        for w in (w1f, w2, w3, w4f):
            fwd += [as_bytes(part) for part in split_hl(FD._swizzle_rows(FD._permute_blocks(w)))]
        fwd.append(as_bytes(torch.cat([b1, b2, b3, b4f])))
        w4t = torch.zeros(32, 128, device=dev); w4t[:w4.shape[0]] = w4
        w4p = torch.zeros(128, FD.ROW4T, device=dev); w4p[:, :32] = FD._permute_blocks(w4t.t().contiguous())
        bwd += [as_bytes(part) for part in split_hl(w4p)]
        for w in (w3, w2, w1f):
            bwd += [as_bytes(part) for part in split_hl(FD._swizzle_rows(FD._permute_blocks(w.t().contiguous())))]
    return torch.cat(fwd), torch.cat(bwd)
