"""GPU tests of the fused decoder for the `sequential` and `parallel` decoder types (chains 1 and 2 of csrc/ggd_mlp.hip,
DESIGN.md section 6r), both precision tiers, and of chain 0 through the chain-taking entry points.

Criterion: DESIGN.md section 6l, unchanged -- the checker is tests/test_decoder_backward_gpu.py's own (_check: a kernel's error
within max(bar, 4 dev), dev = the tier's restatement against float64, never a figure from the kernel; forward bars 2e-3 / 1e-4
of the output scale, relative-L2 bars 1.5e-2 / 1e-3; dfeat per row, parameters elementwise and in L2, dout / dinfo with the
floor 2^-20 max|ref|; no row and no tensor left out; the error / dev ratios printed).  The restatement is
tests/_decoder_chain_ref.py (float64 autograd of the modules, and decoder_ref for chain 0: tests/test_decoder_chains_host.py).
Per-head quantities (dout, the 40 gradients) are indexed by EXECUTION POSITION: for chains 1 and 2 that is xyz, scale,
rotation, opacity, colour -- the order of the modules' own parameters()."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _decoder_chain_raw as CRAW
import _decoder_chain_ref as CR
import _decoder_raw as RAW
import test_decoder_backward_gpu as CRIT     # the criterion: _check, the bars

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TIERS = ("bf16", "fp32")
CHAINS = (1, 2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = {1: "forward_chain_decoder_fixture.npz", 2: "parallel_decoder_fixture.npz"}
_maxabs = CRIT._maxabs


@functools.lru_cache(maxsize=None)
def _module(chain):
    return CR.make_decoder(chain).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(n, only=None):
    """(feats, pos, dattrs) fp32 on the device; only: the attribute (0 colour .. 4 xyz) the loss is on, None: all"""
    feats, pos, dattrs = CR.make_inputs(n)
    if only is not None:
        dattrs = CR.only(dattrs, only)
    return feats.to(DEV), pos.to(DEV), dattrs.to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(chain, n, only=None, tier=None):
    """The float64 restatement (tier None) or a tier's, on the device, computed once per (chain, size, pattern, tier)"""
    feats, pos, dattrs = _inputs(n, only)
    with torch.no_grad():
        return CR.decoder_chain_ref(chain, CR.module_params(_module(chain), chain, torch.float64), feats.double(), pos.double(),
                                    dattrs.double(), CR.IDENTITY if tier is None else CR.TIERS[tier])


def _check(chain, tier, n, got, what, only=None, **kw):
    return CRIT._check(tier, _ref(chain, n, only), _ref(chain, n, only, tier), got, f"chain {chain} {what}", **kw)


def _autograd(chain, precision, feats, pos, dattrs, scenes=None):
    """FusedTrainDecoder forward + backward under the loss sum(attrs * dattrs) -> attrs, dfeat (= feats.grad), grads"""
    from gaussian_gan_decoder_amd.fused_decoder import FusedTrainDecoder
    mod = _module(chain)
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
    grads = [p.grad.clone() for p in mod.parameters()]     # definition order == execution order
    for p in mod.parameters():
        p.grad = None
    return SimpleNamespace(attrs=attrs.detach(), dfeat=f.grad, grads=grads)


@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("chain", CHAINS)
def test_reference_class_fixtures(native_lib, chain, precision):
    """FusedDecoder(SequentialDecoder / ParallelDecoder)(planes, positions), N = 96, against the outputs of the REFERENCE's classes
    (tests/golden/{forward_chain,parallel}_decoder_fixture.npz) within the tier's forward bar of the output scale."""
    from gaussian_gan_decoder_amd.fused_decoder import FusedDecoder
    base = np.load(os.path.join(GOLDEN, "sequential_decoder_fixture.npz"))
    f = np.load(os.path.join(GOLDEN, FIXTURE[chain]))
    dec = CR.module_class(chain)()
    missing, unexpected = dec.load_state_dict({k[3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd_")}, strict=False)
    assert not unexpected and not [m for m in missing if "decoder" in m], (missing, unexpected)
    out = FusedDecoder(dec.to(DEV), precision=precision)(torch.from_numpy(base["planes"]).to(DEV), torch.from_numpy(base["positions"]).to(DEV))
    for k in ("color", "opacity", "rotation", "scale", "xyz"):
        want = torch.from_numpy(f[k])
        err = _maxabs(getattr(out, k).cpu() - want)
        print(f"\n  fixture chain {chain} {precision} {k}: max |err| {err:.3e}, scale {_maxabs(want):.3f}")
        assert err <= CRIT.FWD_BAR[precision] * max(1.0, _maxabs(want)), (k, err)


@pytest.mark.parametrize("n", [1, 17, 33, 257, 4099])
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("chain", CHAINS)
def test_sizes(native_lib, chain, precision, n):
    """A lone point, both edges of a 16-point block and of a 32-point slab, a second backward batch (257), several slabs per wave
    (4099), through FusedTrainDecoder: attrs, dfeat per row and all 40 gradients.  (The granularity of the sizes themselves is
    chain 0's test_sizes_at_every_granularity.)"""
    feats, pos, dattrs = _inputs(n)
    _check(chain, precision, n, _autograd(chain, precision, feats, pos, dattrs), f"sizes N={n}")


@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("chain", CHAINS)
def test_raw_entry_points(native_lib, chain, precision):
    """The *_chain entry points, N = 257: + dout [5,N,4] by execution position and dinfo [N,16] in the chain's slot order."""
    n = 257
    got = CRAW.run(_module(chain), *_inputs(n), precision=precision)
    _check(chain, precision, n, got, f"raw N={n}", raw=True)
    if chain == 2:      # nobody reads an earlier head: only the position's gradient is carried
        assert torch.count_nonzero(got.dinfo[:, 3:]).item() == 0


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("chain", CHAINS)
def test_poisoned_attrs(native_lib, chain, precision, n):
    """Production allocates attrs with torch.empty, and the new chains write its columns out of column order: a head must never
    read a column no earlier head wrote.  attrs filled with NaN before the forward: every output finite and bit-equal to the run
    on a zeroed buffer."""
    ins = _inputs(n)
    clean = CRAW.run(_module(chain), *ins, precision=precision, attrs_fill=0.0)
    got = CRAW.run(_module(chain), *ins, precision=precision, attrs_fill=float("nan"))
    for name in ("attrs", "dfeat", "dinfo", "dout", "wg"):
        a, b = getattr(got, name), getattr(clean, name)
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name     # (wg too: at these sizes one weight-gradient workgroup per (head, layer), one order of its atomics)
    assert torch.equal(RAW.rows(got.zbuf)[:, :n], RAW.rows(clean.zbuf)[:, :n])
    assert torch.equal(RAW.rows(got.dzbuf)[:, :n], RAW.rows(clean.dzbuf)[:, :n])
    _check(chain, precision, n, got, f"poisoned attrs N={n}", raw=True)


@pytest.mark.parametrize("precision", TIERS)
def test_parallel_chain_has_no_cross_talk(native_lib, precision):
    """Chain 2, loss on colour only, N = 257: the 32 parameter tensors of the other four heads (execution positions 0..3) are
    exactly zero and finite; dfeat and the colour head's gradients meet the criterion."""
    n = 257
    got = CRAW.run(_module(2), *_inputs(n, 0), precision=precision)
    for k, g in enumerate(got.grads[:32]):
        assert torch.isfinite(g).all() and torch.count_nonzero(g).item() == 0, k
    assert torch.count_nonzero(got.dout[:4]).item() == 0
    _check(2, precision, n, got, f"colour only N={n}", only=0, heads=(4,), raw=True)


@pytest.mark.parametrize("precision", TIERS)
def test_sequential_chain_loss_on_one_attribute(native_lib, precision):
    """Chain 1, N = 257.  Loss on xyz only (the FIRST head): every later head's gradients are exactly zero.  Loss on colour only
    (the LAST head): all five heads receive gradient through the chained inputs, within the criterion."""
    n = 257
    got = CRAW.run(_module(1), *_inputs(n, 4), precision=precision)
    for k, g in enumerate(got.grads[8:], 8):
        assert torch.isfinite(g).all() and torch.count_nonzero(g).item() == 0, k
    assert torch.count_nonzero(got.dout[1:]).item() == 0
    _check(1, precision, n, got, f"xyz only N={n}", only=4, heads=(0,), raw=True)
    got = CRAW.run(_module(1), *_inputs(n, 0), precision=precision)
    assert all(torch.count_nonzero(g).item() > 0 for g in got.grads)
    _check(1, precision, n, got, f"colour only N={n}", only=0, raw=True)


@pytest.mark.parametrize("precision", TIERS)
def test_chain_0_through_the_chain_entry_points(native_lib, precision):
    """ggd_decoder_*_chain(GGD_CHAIN_SEQUENTIAL_REVERSED, ...) against the entry points without a chain, N = 1000: both weight
    images, attrs, z, dfeat, dinfo, dout and dz bit for bit with chunk = 0; and with chunk = 256 -- every launch pair then has ONE
    weight-gradient workgroup per (head, layer) and the launches are ordered by the stream, so the float atomics have one order
    -- the weight gradients bit for bit too."""
    import _decoder_ref as R
    n = 1000
    mod = R.make_decoder().to(DEV)
    ins = tuple(t.to(DEV) for t in R.make_inputs(n))
    for chunk in (0, 256):
        old = CRAW.run(mod, *ins, precision=precision, chunk=chunk, entry="plain")
        new = CRAW.run(mod, *ins, precision=precision, chunk=chunk, entry="chain")
        for name in ("packed", "packed_t", "attrs", "dfeat", "dinfo", "dout") + (("wg",) if chunk else ()):
            assert torch.equal(getattr(old, name), getattr(new, name)), (chunk, name)
        assert torch.equal(old.zbuf, new.zbuf) and torch.equal(old.dzbuf, new.dzbuf), chunk
        assert torch.isfinite(new.wg).all() and _maxabs(old.wg - new.wg) <= 1e-5 * _maxabs(old.wg)
    base = RAW.run(mod, *ins, precision=precision)           # what FusedDecoderFn did before the chains
    assert torch.equal(base.attrs, new.attrs) and torch.equal(base.dfeat, new.dfeat)


@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("chain", CHAINS)
def test_forward_scenes_equals_separate_scenes(native_lib, chain, precision):
    """forward_scenes (B = 3 scenes of 333 points through one launch): attrs equal three separate forward calls -- bit for bit in
    the bf16 tier, within the forward bar at reference precision -- and feats.grad per row and the parameter gradients meet the
    criterion against the float64 restatement of the 999 points."""
    from gaussian_gan_decoder_amd.fused_decoder import FusedTrainDecoder
    B, n = 3, 333
    feats, pos, dattrs = _inputs(B * n)
    got = _autograd(chain, precision, feats, pos, dattrs, scenes=B)
    fused = FusedTrainDecoder(_module(chain), precision)
    with torch.no_grad():
        for b in range(B):
            s = slice(b * n, (b + 1) * n)
            o = fused(None, pos[s].clone(), features=feats[s].clone())
            one = torch.cat([o.color, o.opacity, o.rotation, o.scale, o.xyz], 1)
            if precision == "bf16":
                assert torch.equal(one, got.attrs[s, :14]), b
            else:
                assert _maxabs(one - got.attrs[s, :14]) <= CRIT.FWD_BAR[precision] * max(1.0, _maxabs(one)), b
    _check(chain, precision, B * n, got, f"forward_scenes B={B} N={n}")


def test_unknown_chain_is_refused(native_lib):
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(torch.device(DEV))
    z = C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    for chain in (-1, 3):
        assert cx.lib.ggd_decoder_forward_chain(cx.handle, st, chain, z, z, 16, z, z) != 0
        assert b"unknown decoder chain" in cx.lib.ggd_last_error(cx.handle)
        assert cx.lib.ggd_decoder_pack_hl_chain(cx.handle, st, chain, None, z, z) != 0
        assert cx.lib.ggd_decoder_backward_wgrad_chain(cx.handle, st, chain, 16, 0, z, z, z, z, z, z, z, z, z, z, z) != 0
        assert b"unknown decoder chain" in cx.lib.ggd_last_error(cx.handle)


@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("decoder_type", ["sequential", "parallel"])
def test_one_trainer_step(native_lib, decoder_type, precision):
    """DecoderTrainer(decoder_type=t, fused_decoder=True) against the same trainer with the PyTorch decoder (same seed, same
    batch: 2 scenes x 2048 points, 64 x 64 image, no perceptual term, no backbone stand-in, the decoder as the trainer
    initialises it): the step-0 loss within the tier's relative-L2 bar of the PyTorch trainer's, and EVERY decoder parameter
    tensor's gradient within it in relative L2 (per tensor, as section 6l states its bars; every tensor must carry a gradient).

    Measured (one MI355X; profiles/r09/trainer_step.txt), worst tensor, bf16 / fp32: sequential 9.82e-3 / 9.03e-4, parallel
    1.26e-2 / 9.92e-4 (bars 1.5e-2 / 1e-3); loss 8.5e-5 / 7.0e-7 and 1.0e-5 / 3.7e-7.  The worst tensors are the xyz head's, and
    what they show is the tier's own rounding: at the fused trainer's own feats / pos / dattrs the kernels lie as far from the
    float64 restatement as the tier's restatement does (9.914e-4 against 9.934e-4 for the closest case).  The figure depends on
    the scene: with the output biases of tests/test_train_step_gpu.py (scale + 3.5, opacity + 1: large splats, the loss on few
    points) the same tensors reach 1.6e-2 - 2.5e-2 / 1.9e-3 - 2.3e-3, chain 0 included, still equal to the restatement's own
    deviation."""
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    dev = torch.device(DEV)

    def make(fused):
        return DecoderTrainer(dev, n_scenes_total=2, plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7,
                              perceptual_weight=0.0, backbone_params=0, decoder_type=decoder_type, fused_decoder=fused,
                              decoder_precision=precision)

    def half_step(tr):
        tr.flat_grad.zero_()
        loss = tr.local_loss(make_scene_batch([0, 1], 2048, 64, dev, seed=0))
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach())
    ref_tr, tr = make(False), make(True)
    assert all(torch.equal(a, b) for a, b in zip(ref_tr.params, tr.params))
    l0, l1 = half_step(ref_tr), half_step(tr)
    bar = CRIT.L2_BAR[precision]
    print(f"\n  trainer {decoder_type} {precision}: loss {l0:.6f} (PyTorch) {l1:.6f} (fused), relative {abs(l1 - l0) / abs(l0):.2e}")
    worst, bad, off = 0.0, [], 0
    g0, g1 = ref_tr.flat_grad.detach(), tr.flat_grad.detach()
    assert torch.isfinite(g1).all()
    names = [n for n, _ in ref_tr.decoder.named_parameters()]
    by_id = {id(p): n for n, p in ref_tr.decoder.named_parameters()}
    for p in ref_tr.params:
        k = p.numel()
        if id(p) in by_id:
            a, b = g0[off:off + k], g1[off:off + k]
            assert float(a.norm()) > 0, by_id[id(p)]
            rel = float((a - b).norm() / a.norm())
            worst = max(worst, rel)
            if not rel <= bar:
                bad.append((by_id[id(p)], rel))
        off += k
    assert len(names) == 40
    print(f"  trainer {decoder_type} {precision}: worst relative L2 of a decoder parameter gradient {worst:.3e} (bar {bar:.1e})")
    assert abs(l1 - l0) <= bar * abs(l0), (l0, l1)
    assert not bad, bad
