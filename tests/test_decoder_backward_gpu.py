"""GPU tests of the fused decoder's training backward (decoder_backward_kernel, decoder_wgrad_kernel and their reference-
precision twins, csrc/ggd_mlp_bwd.inc / ggd_mlp_wgrad.inc / ggd_mlp_hl.inc) per point and per element, at every granularity
of the kernels, in chunks, through the split entry points, over poisoned padding rows and with zero gradients.

Criterion.  The yardstick of a quantity q is dev(q): how far the tier's restatement with the kernels'
rounding points (tests/_decoder_ref.py: BF16_TIER / FP32_TIER, float64 sums) lies from the float64 restatement on the
same inputs -- computed here from the reference, never from the kernel.  A kernel rounds where its restatement rounds and sums in
another order, so its error must stay within max(bar, 4 * dev) (the factor the masked-loss tests use for "same rounding points,
different summation order"); bar is the project's existing figure where there is one (relative L2 of a parameter gradient:
1.5e-2 / 1e-3; forward outputs: 2e-3 / 1e-4 of the output scale) and 0 elsewhere:
  * attrs      per head, max |err| against max(bar * max(1, max|ref|), 4 dev)
  * dfeat      PER ROW: max |err| over the row against 4 R max|row64|, R = the largest dev_row / max|row64| of any row
  * parameters per tensor, max |err| elementwise against 4 max|dev|, and relative L2 against max(bar, 4 dev_L2)
  * dout, dinfo (raw calls) per tensor, max |err| against max(4 max|dev|, 2^-20 max|ref|): the restatements run in float64 and
    model no fp32 arithmetic, and the xyz head's dout = 0.01 dattrs has no rounding point at all -- 2^-20 is four ulps of
    the largest element for the kernels' own fp32 multiply / expf there
No row and no tensor is left out.  Every test prints the ratio of the kernel's error to dev for each quantity."""
import functools
from types import SimpleNamespace

import pytest
import torch

import _decoder_raw as RAW
import _decoder_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FACTOR = 4.0
L2_BAR = {"bf16": 1.5e-2, "fp32": 1e-3}
FWD_BAR = {"bf16": 2e-3, "fp32": 1e-4}
TIERS = ("bf16", "fp32")
SIZES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 4099, 70001)


@functools.lru_cache(maxsize=None)
def _module():
    return R.make_decoder().to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(n, kind="full"):
    """(feats, pos, dattrs) fp32 on the device; kind: "full", "dead" (zero_point_mask rows of dattrs zero), "colour" """
    feats, pos, dattrs = R.make_inputs(n)
    if kind == "dead":
        dattrs[R.zero_point_mask(n)] = 0
    elif kind == "colour":
        dattrs = R.colour_only(dattrs)
    return feats.to(DEV), pos.to(DEV), dattrs.to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(n, kind="full", tier=None):
    """The float64 restatement (tier None) or a tier's, on the device, computed once per (size, pattern, tier)"""
    feats, pos, dattrs = _inputs(n, kind)
    with torch.no_grad():
        return R.decoder_ref(R.module_params(_module(), torch.float64), feats.double(), pos.double(), dattrs.double(),
                             R.IDENTITY if tier is None else R.TIERS[tier])


def _maxabs(t):
    return t.abs().max().item() if t.numel() else 0.0


def _check(tier, ref, pre, got, what, rows=None, heads=range(5), raw=False, forward=True):
    """Every quantity of `got` (attrs, dfeat, grads; raw: + dout, dinfo) against the criterion; prints the kernel-error / dev
    ratios; rows: bool mask of the dfeat rows that carry a gradient (the others are the caller's to check); heads: whose
    parameter gradients are compared.  Collects every miss before it fails."""
    bad, ratio = [], {}

    def note(q, err, dev):
        ratio[q] = max(ratio.get(q, 0.0), err / dev if dev > 0 else (float("inf") if err > 0 else 0.0))

    if forward:
        for h in range(5):
            c = slice(R.A0[h], R.A0[h] + R.OD[h])
            err, dev = _maxabs(got.attrs[:, c].double() - ref.attrs[:, c]), _maxabs(pre.attrs[:, c] - ref.attrs[:, c])
            note("attrs", err, dev)
            if not err <= max(FWD_BAR[tier] * max(1.0, _maxabs(ref.attrs[:, c])), FACTOR * dev):
                bad.append((f"attrs head {h}", err, dev))
        assert _maxabs(got.attrs[:, 14:]) == 0.0
    # dfeat, per row
    sel = torch.ones(ref.dfeat.shape[0], dtype=torch.bool, device=ref.dfeat.device) if rows is None else rows
    rowmax = ref.dfeat.abs().amax(1)[sel]
    assert (rowmax > 0).all()
    Rdev = ((pre.dfeat - ref.dfeat).abs().amax(1)[sel] / rowmax).max().item()
    rerr = (got.dfeat.double() - ref.dfeat).abs().amax(1)[sel] / rowmax
    assert torch.isfinite(got.dfeat).all()
    note("dfeat_row", rerr.max().item(), Rdev)
    if not bool((rerr <= FACTOR * Rdev).all()):
        bad.append(("dfeat rows", int((rerr > FACTOR * Rdev).sum()), rerr.max().item(), Rdev))
    if raw:
        for name, g, r, p in [(f"dout head {h}", got.dout[h], ref.dout[h], pre.dout[h]) for h in range(5)] + \
                             [("dinfo", got.dinfo, ref.dinfo, pre.dinfo)]:
            assert torch.isfinite(g).all(), name
            err, dev, floor = _maxabs(g.double() - r), _maxabs(p - r), 2.0 ** -20 * _maxabs(r)
            note(name.split()[0], err, max(dev, floor))
            if not err <= max(FACTOR * dev, floor):
                bad.append((name, err, dev))
    for h in heads:
        for k in range(8 * h, 8 * h + 8):
            g, r, p = got.grads[k], ref.grads[k], pre.grads[k]
            assert g is not None and g.shape == r.shape and torch.isfinite(g).all(), k
            err, dev = _maxabs(g.double() - r), _maxabs(p - r)
            note("param_max", err, dev)
            if not err <= FACTOR * dev:
                bad.append((f"parameter {k} elementwise", err, dev))
            l2, dl2 = ((g.double() - r).norm() / r.norm()).item(), ((p - r).norm() / r.norm()).item()
            note("param_l2", l2, dl2)
            if not l2 <= max(L2_BAR[tier], FACTOR * dl2):
                bad.append((f"parameter {k} relative L2", l2, dl2))
    print(f"\n  RATIO {tier} {what}: " + "  ".join(f"{q} {v:.2f}" for q, v in ratio.items()))
    assert not bad, bad
    return ratio


def _autograd(precision, feats, pos, dattrs, scenes=None):
    """FusedTrainDecoder forward + backward under the loss sum(attrs * dattrs) -> attrs, dfeat (= feats.grad), grads"""
    from gaussian_gan_decoder_amd.fused_decoder import FusedTrainDecoder
    mod = _module()
    for p in mod.parameters():
        p.grad = None
    fused = FusedTrainDecoder(mod, precision)
    f = feats.clone().requires_grad_(True)
    if scenes is None:
        o = fused(None, pos, features=f)
        attrs = torch.cat([o.color, o.opacity, o.rotation, o.scale, o.xyz, torch.zeros_like(o.xyz[:, :2])], 1)
        (attrs[:, :14] * dattrs[:, :14]).sum().backward()
    else:
        attrs = fused.forward_scenes(None, pos.view(scenes, -1, 3), feats=f).reshape(-1, 16)
        (attrs * dattrs).sum().backward()
    grads = [p.grad.clone() for p in mod.parameters()]
    for p in mod.parameters():
        p.grad = None
    return SimpleNamespace(attrs=attrs.detach(), dfeat=f.grad, grads=grads)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("precision", TIERS)
def test_sizes_at_every_granularity(native_lib, precision, n):
    """16 points (a block of the Z layout), 32 (a slab and its fp16 scale), 64 (a weight-gradient stage), 256 (a backward
    workgroup batch), each at -1, 0, +1; 4099; and 70 001, past both grid caps (256 backward workgroups, 128 split-K chunks):
    there per = 288, so one wave of every backward workgroup runs a second slab, and a weight-gradient workgroup runs 9 stages."""
    feats, pos, dattrs = _inputs(n)
    got = _autograd(precision, feats, pos, dattrs)
    _check(precision, _ref(n), _ref(n, "full", precision), got, f"sizes N={n}")


@functools.lru_cache(maxsize=None)
def _unchunked(precision, n):
    return RAW.run(_module(), *_inputs(n), precision=precision, chunk=0)


def _same_bits(a, b, n, what):
    for name in ("attrs", "dfeat", "dinfo", "dout"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert torch.equal(RAW.rows(a.dzbuf)[:, :n], RAW.rows(b.dzbuf)[:, :n]), (what, "dzbuf")
    assert torch.equal(RAW.rows(a.zbuf)[:, :n], RAW.rows(b.zbuf)[:, :n]), (what, "zbuf")


@pytest.mark.parametrize("n,chunk", [(1000, c) for c in (1, 256, 300, 512, 999, 1000, 1001)] + [(70001, 4096), (70001, 65536)])
@pytest.mark.parametrize("precision", TIERS)
def test_chunked_equals_unchunked(native_lib, precision, n, chunk):
    """ggd_decoder_backward_wgrad(_hl) with a non-zero chunk (rounded up to 256: 1 -> 256, 300 -> 512, 999 -> 1024 = one chunk):
    dfeat, dinfo, dout and the first N rows of every dz plane equal the chunk = 0 run BIT FOR BIT -- bf16: every point is computed
    on its own; reference precision: chunk boundaries are multiples of 256, so every 32-point slab and its scale are unchanged
    -- and the weight gradients (float atomics: not bitwise) meet the criterion against float64, although the weight-gradient
    launch of a chunk reads the head's largest exponent before later chunks have raised it."""
    base = _unchunked(precision, n)
    got = RAW.run(_module(), *_inputs(n), precision=precision, chunk=chunk)
    _same_bits(got, base, n, f"chunk {chunk}")
    _check(precision, _ref(n), _ref(n, "full", precision), got, f"chunk N={n} chunk={chunk}", raw=True)


@pytest.mark.parametrize("precision", TIERS)
def test_chunked_through_autograd(native_lib, precision, monkeypatch):
    """fused_decoder.WGRAD_CHUNK (GGD_WGRAD_CHUNK) = 300 through FusedDecoderFn: the same feats.grad bits, gradients within
    the criterion."""
    from gaussian_gan_decoder_amd import fused_decoder
    n = 1000
    feats, pos, dattrs = _inputs(n)
    monkeypatch.setattr(fused_decoder, "WGRAD_CHUNK", 0)
    base = _autograd(precision, feats, pos, dattrs)
    monkeypatch.setattr(fused_decoder, "WGRAD_CHUNK", 300)
    got = _autograd(precision, feats, pos, dattrs)
    assert torch.equal(got.attrs, base.attrs) and torch.equal(got.dfeat, base.dfeat)
    _check(precision, _ref(n), _ref(n, "full", precision), got, f"autograd chunk=300 N={n}")


def test_split_entry_points(native_lib):
    """ggd_decoder_backward followed by ggd_decoder_wgrad (bf16 tier; documented as ggd_decoder_backward_wgrad with chunk <= 0,
    called by nobody else): the same dfeat / dinfo / dout / dz bits, weight gradients within the criterion."""
    n = 1000
    got = RAW.run(_module(), *_inputs(n), precision="bf16", split=True)
    _same_bits(got, _unchunked("bf16", n), n, "split")
    _check("bf16", _ref(n), _ref(n, "full", "bf16"), got, f"split N={n}", raw=True)


@pytest.mark.parametrize("n", [1, 17, 33, 1001])
@pytest.mark.parametrize("precision", TIERS)
def test_poisoned_padding_rows(native_lib, precision, n):
    """zbuf and dzbuf are torch.empty in production and the rows between N and the next multiple of 16 are never written: the
    kernels' masks must keep them out of the MFMAs (a stale NaN times a zero operand is a NaN in dW).  Both buffers pre-filled
    with 0xFF bytes (NaN as f16 and as bf16): every output finite and within the criterion, dfeat / dinfo / dout and the written
    rows equal to the zero-filled run bit for bit, the padding rows untouched."""
    ins = _inputs(n)
    clean = RAW.run(_module(), *ins, precision=precision, zbuf=RAW.planes(n, 0), dzbuf=RAW.planes(n, 0))
    got = RAW.run(_module(), *ins, precision=precision, zbuf=RAW.planes(n, -1), dzbuf=RAW.planes(n, -1))
    for g in got.grads:
        assert torch.isfinite(g).all()
    _same_bits(got, clean, n, "poisoned")
    for name in ("zbuf", "dzbuf"):
        pad = RAW.rows(getattr(got, name))[:, n:]
        assert pad.shape[1] == (-n) % 16 and bool((pad == -1).all()), name
        assert bool((RAW.rows(getattr(clean, name))[:, n:] == 0).all()), name
    _check(precision, _ref(n), _ref(n, "full", precision), got, f"poisoned N={n}", raw=True)


def test_points_do_not_depend_on_their_neighbours(native_lib):
    """bf16 tier: rows [:33] of attrs, dfeat, dinfo and dout from a run at N = 257 equal the run on the first 33 points alone, bit
    for bit (the backward counterpart of test_exploding_preactivation_stays_inside_its_point)."""
    feats, pos, dattrs = _inputs(257)
    big = RAW.run(_module(), feats, pos, dattrs, precision="bf16")
    small = RAW.run(_module(), feats[:33].clone(), pos[:33].clone(), dattrs[:33].clone(), precision="bf16")
    assert torch.equal(big.attrs[:33], small.attrs) and torch.equal(big.dfeat[:33], small.dfeat)
    assert torch.equal(big.dinfo[:33], small.dinfo) and torch.equal(big.dout[:, :33], small.dout)
    assert torch.equal(RAW.rows(big.dzbuf)[:, :33], RAW.rows(small.dzbuf)[:, :33])


@pytest.mark.parametrize("precision", TIERS)
def test_points_without_a_gradient(native_lib, precision):
    """Culled Gaussians: dattrs zero for points 64..159 (three whole slabs: the reference-precision tier's "no gradient in this
    slab" path, scale factors 0) and for every third point elsewhere.  Their dfeat / dinfo / dout rows are EXACTLY zero (the
    float64 restatement's are: test_decoder_ref_host.py), everything else meets the criterion."""
    n = 1000
    dead = R.zero_point_mask(n).to(DEV)
    got = RAW.run(_module(), *_inputs(n, "dead"), precision=precision)
    assert torch.count_nonzero(got.dfeat[dead]).item() == 0 and torch.count_nonzero(got.dinfo[dead]).item() == 0
    assert torch.count_nonzero(got.dout[:, dead]).item() == 0
    assert torch.count_nonzero(RAW.rows(got.dzbuf)[:, :n][:, dead] & 0x7FFF).item() == 0      # +-0 in either 16-bit format
    _check(precision, _ref(n, "dead"), _ref(n, "dead", precision), got, f"dead points N={n}", rows=~dead, raw=True)


@pytest.mark.parametrize("chunk", [0, 256])
@pytest.mark.parametrize("precision", TIERS)
def test_loss_on_colour_only(native_lib, precision, chunk):
    """The other four heads get no gradient at all: their 32 parameter gradients are exactly zero and finite (reference
    precision: the early return on the memset pattern of the per-head exponent -- with chunk = 256 in every launch), the
    colour head's meet the criterion."""
    n = 1000
    got = RAW.run(_module(), *_inputs(n, "colour"), precision=precision, chunk=chunk)
    for k, g in enumerate(got.grads[8:], 8):
        assert torch.isfinite(g).all() and torch.count_nonzero(g).item() == 0, k
    assert torch.count_nonzero(got.dout[1:]).item() == 0
    _check(precision, _ref(n, "colour"), _ref(n, "colour", precision), got, f"colour only N={n} chunk={chunk}", heads=(0,), raw=True)


@pytest.mark.parametrize("precision", TIERS)
def test_forward_scenes_equals_separate_scenes(native_lib, precision):
    """forward_scenes (B = 3 scenes of 333 points through one launch): attrs equal three separate forward calls -- bit for bit in
    the bf16 tier, within the forward bar at reference precision -- and feats.grad per row and the parameter gradients meet the
    criterion against the float64 restatement of the 999 points (= the sum over the scenes)."""
    from gaussian_gan_decoder_amd.fused_decoder import FusedTrainDecoder
    B, n = 3, 333
    feats, pos, dattrs = _inputs(B * n)
    got = _autograd(precision, feats, pos, dattrs, scenes=B)
    fused = FusedTrainDecoder(_module(), precision)
    with torch.no_grad():
        for b in range(B):
            s = slice(b * n, (b + 1) * n)
            o = fused(None, pos[s].clone(), features=feats[s].clone())
            one = torch.cat([o.color, o.opacity, o.rotation, o.scale, o.xyz], 1)
            if precision == "bf16":
                assert torch.equal(one, got.attrs[s, :14]), b
            else:
                assert _maxabs(one - got.attrs[s, :14]) <= FWD_BAR[precision] * max(1.0, _maxabs(one)), b
    _check(precision, _ref(B * n), _ref(B * n, "full", precision), got, f"forward_scenes B={B} N={n}")
